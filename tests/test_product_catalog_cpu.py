"""The product catalog (tests/product_catalog.py) against the product kernels csrc/sparse.hip instantiates and against the
host restatement of its dispatch (product_catalog.product_plan), and the two numpy restatements of the kernels'
summation order against scipy -- host only."""
import os
import re
import numpy as np
import pytest
from scipy import sparse

from product_catalog import BY_NAME, CASES, PRODUCT_VARIANTS, all_targets, product_plan, restated_real, widths_planned
from test_complex_cpu import restated_product

IDS = [c.name for c in CASES]


def test_product_catalog_covers_every_variant():
    """every product kernel the library instantiates is a target of some case, and nothing else is named; the table is
    read off the launch sites of sparse.hip, so a dispatch change that adds or drops an instantiation fails here until
    the catalog follows"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eigd_amd", "csrc", "sparse.hip")).read()
    host = src[src.index('extern "C"'):]
    inst = lambda macro: [int(v) for v in re.findall(macro + r"\((\d+)\)\n", host)]      # noqa: E731
    found = (["spmv_stream_kernel"] + [f"spmm_tiled_kernel<{kp}, 8>" for kp in inst("EIGD_SPMM_TILED")]
             + [f"spmm_tiled_kernel<{kp}, 8, true>" for kp in inst("EIGD_SPMM_DOTS")] + ["tile_dots_reduce_kernel"]
             + [f"spmm_rows_kernel<{kp}>" for kp in inst("EIGD_SPMM_CASE")]
             + ["cspmv_stream_kernel", "cspmm_tiled_kernel<true>", "cspmm_tiled_kernel<false>"])
    for name in ("spmv_stream_kernel", "tile_dots_reduce_kernel", "cspmv_stream_kernel", "cspmm_tiled_kernel<true>",
                 "cspmm_tiled_kernel<false>"):
        assert "hipLaunchKernelGGL(" + name in host, name
    assert found == PRODUCT_VARIANTS
    table = PRODUCT_VARIANTS
    assert len(table) == len(set(table)) == 20
    targets = all_targets()
    missing, unknown = set(table) - targets, targets - set(table)
    assert not missing, f"variants no catalog case launches: {sorted(missing)}"
    assert not unknown, f"catalog names variants the library does not have: {sorted(unknown)}"
    assert len(IDS) == len(set(IDS))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planned_launches_hold_every_target(case):
    """the plan of every width the case runs covers the block's columns once, in order, with kernels of the table; all
    plans together hold the case's (variant, columns) targets; the statistics are the ones the case claims"""
    A = case.build()
    table = set(PRODUCT_VARIANTS)
    planned = set()
    for kind, k, unit in widths_planned(case):
        plan, stats = product_plan(A, k, kind, unit_ld=unit)
        products = [(v, c0, nc) for v, c0, nc in plan if v != "tile_dots_reduce_kernel"]
        assert {v for v, _, _ in plan} <= table
        assert [c0 for _, c0, _ in products] == list(np.cumsum([0] + [nc for _, _, nc in products[:-1]]))
        assert sum(nc for _, _, nc in products) == k
        assert stats["fused_dots"] == any("true>" in v and v.startswith("spmm_tiled") for v, _, _ in plan)
        assert stats["fused_dots"] == any(v == "tile_dots_reduce_kernel" for v, _, _ in plan)
        for name, want in case.stats.items():
            assert stats[name] == want, (case.name, kind, k, name, stats)
        planned |= {(v, nc) for v, _, nc in plan}
    missing = [t for t in case.targets if t not in planned]
    assert not missing, f"{case.name}: not planned {missing}; planned {sorted(planned)}"


def test_branch_counts_of_the_mixed_and_the_edge_cases():
    _, st = product_plan(BY_NAME["band20_thin"].build(), 32)
    assert (st["tiles"] - st["direct_tiles"], st["direct_tiles"]) == (2, 32)        # one launch mixes both
    A = BY_NAME["row_block_edges"].build()
    ln = np.diff(A.indptr)
    assert ln[1] == 2046 and ln[2] == 2047 and A.indptr[1] % 2 == 1 and not ln[3:303].any()
    _, st = product_plan(A, 1, unit_ld=True)
    assert st["long_row_blocks"] == 1
    # rows 0 | 1 | 2 | 256 empty rows | the other 44 empty rows and the 2297 rows of the tail, 256 rows a block
    assert st["row_blocks"] == 3 + 1 + -(-(44 + 2297) // 256)
    _, st = product_plan(A.astype(complex), 1, "complex")
    assert st["long_row_blocks"] == 0                        # the complex stream kernel stages up to 2048 non-zeros
    A = BY_NAME["carrow4230"].build()
    assert np.diff(A.indptr).max() == 4200                   # three chunks of 2048
    A = BY_NAME["tridiag_131105"].build()
    _, st = product_plan(A, 32, "cg")
    assert st["tiles"] > 1024 * (256 // 64)                  # tile_dots_reduce_kernel: a second trip at 32 columns


def test_product_plan_follows_its_inputs():
    A = BY_NAME["grid"].build()
    plan = lambda *a, **kw: product_plan(A, *a, **kw)[0]    # noqa: E731
    assert plan(32) == [("spmm_tiled_kernel<32, 8>", 0, 32)]
    assert plan(33) == [("spmm_tiled_kernel<32, 8>", 0, 32), ("spmm_tiled_kernel<2, 8>", 32, 1)]
    assert plan(1, unit_ld=True) == [("spmv_stream_kernel", 0, 1)]
    assert plan(1) == [("spmm_tiled_kernel<2, 8>", 0, 1)]
    for k in (1, 2, 3, 4, 33, 40, 64):                       # the CG fallback: the plain product's plan
        assert plan(k, "cg") == plan(k) and not product_plan(A, k, "cg")[1]["fused_dots"], k
    for k in (5, 8, 9, 32):
        kp = 8 if k <= 8 else 16 if k <= 16 else 32
        assert plan(k, "cg") == [(f"spmm_tiled_kernel<{kp}, 8, true>", 0, k), ("tile_dots_reduce_kernel", 0, k)]
    assert plan(32, "cg") != plan(32)
    B = BY_NAME["arrow143"].build()                          # the 32-column tile does not fit: no fused dots either
    assert product_plan(B, 32, "cg")[0] == product_plan(B, 32)[0] == [("spmm_rows_kernel<32>", 0, 32)]
    assert product_plan(BY_NAME["arrow142"].build(), 64)[0] == [("spmm_tiled_kernel<32, 8>", 0, 32),
                                                                ("spmm_tiled_kernel<32, 8>", 32, 32)]
    assert product_plan(B, 64)[0] == [("spmm_rows_kernel<64>", 0, 64)]
    assert [nc for _, _, nc in plan(70, "complex")] == [32, 32, 6]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scipy_product_is_the_restatement(case):
    """on every catalog matrix the restatement of the kernels' order (storage order, every multiply and add rounded on
    its own) equals scipy's A @ X bit for bit, at one column (csr_matvec) and at several (csr_matvecs) -- so the GPU
    tests may gate on either.  A case that scipy does not reproduce is marked scipy_bitwise = False"""
    A = case.build()
    rng = np.random.default_rng(11)
    for k in (1, 3):
        X = rng.normal(size=(A.shape[1], k))
        if case.kind == "complex":
            X = X + 1j * rng.normal(size=X.shape)
            assert A.has_sorted_indices
            ours = restated_product(A, X)
        else:
            ours = restated_real(A, X)
        same = np.array_equal(ours.view(np.uint64), np.asarray(A @ X).view(np.uint64))
        assert same == case.scipy_bitwise, (case.name, k)
