"""
Catalog of the triangular sweep's launch variants (csrc/factor.hip, sweep_launches): which small problem makes the
launch policy pick which kernel, at which level of the assembly tree.  Plain data, no GPU import.

Each Case names a matrix builder with its Symbolic parameters, the shift (None: SPD, Cholesky fronts;
"indefinite": between two well-separated eigenvalues, Bunch-Kaufman fronts, TRI = false), the sweep widths it solves,
environment settings, and the (variant, level) pairs its solves must launch (a superset is fine: the record of the
solves is checked to contain them).  ``replicas`` > 1: the matrix is block diagonal, ``replicas`` copies of one
block scaled by powers of four (replica i = 4**scale(i) * A0); levels are heights in the assembly tree, so the same
front of every replica lands on one level, which is how the thresholds on the number of fronts of a level are reached.

The library compiles exactly the variants its launch policy can ask for (factor.hip: sweep_kernels, sweep_launches),
and every one of them is a target here: test_sweep_catalog_covers_every_variant (CPU) checks that the targets are
exactly the library's variant table, so a change of the launch policy that adds or removes a variant fails until this
file is updated.  test_planned_launches_hold_every_target (CPU) asks the policy itself, through Symbolic.sweep_plan,
whether a case's symbolic analysis plans its targets; tests/test_gpu_sweep_variants.py runs the cases and checks that
what ran is what was planned.
"""
from dataclasses import dataclass, field

import numpy as np
from scipy import sparse

from test_gpu_kernels import hub_matrix, lap3d, star_matrix
from test_symbolic_cpu import grid_matrix

KB_OF_KPT = {1: 4, 4: 16, 8: 32}
BIG_LD = (8191, 8192)            # leading dimensions of the 4 GB buffer edge (n = 65536: n * ld * 8 just below / at 2**32)


@dataclass(frozen=True)
class Case:
    name: str
    build: object                        # () -> scipy CSR matrix (SPD, unshifted); with replicas: the block A0
    sym: dict = field(default_factory=dict)
    shift: object = None                 # None or "indefinite"
    widths: tuple = (4, 16, 32)
    env: tuple = ()                      # ((name, value), ...)
    targets: tuple = ()                  # ((variant name, level), ...)
    replicas: int = 1
    reference: str = "splu"              # "splu": scipy's LU of the matrix (of A0 for replicas); "schur": hub problems
    hub: int = 0                         # size of the hub block ("schur" reference)


def scale_exponents(replicas):
    """replica i is 4**m_i * A0: m cycles through -2..2 (exact power-of-two scalings of A0's factor)"""
    return (np.arange(replicas) % 5) - 2


def indefinite_shift(A0):
    """midpoint of the widest gap between two neighbouring eigenvalues in the middle half of A0's spectrum"""
    ev = np.linalg.eigvalsh(A0.toarray())
    lo, hi = len(ev) // 4, 3 * len(ev) // 4
    g = np.argmax(ev[lo + 1:hi] - ev[lo:hi - 1]) + lo
    return 0.5 * (ev[g] + ev[g + 1])


def matrix_of(case):
    """(full matrix, the block A0 the reference factors, shift) -- A0 is the whole matrix unless the case replicates"""
    A0 = case.build().tocsr()
    sigma = indefinite_shift(A0) if case.shift == "indefinite" else 0.0
    if sigma:
        A0 = (A0 - sigma * sparse.identity(A0.shape[0])).tocsr()
    if case.replicas > 1:
        s = 4.0 ** scale_exponents(case.replicas)
        A = sparse.kron(sparse.diags(s), A0).tocsr()
    else:
        A = A0
    A.sort_indices()
    A0.sort_indices()
    return A, A0, sigma


def _thin(KB, nks, nsl, wpf, tri, level):
    return (f"fwd_thin_kernel<{KB}, {nks}, {nsl}, {wpf}, {tri}>", level)


def _both_kb(fn):
    return tuple(t for KB in (16, 32) for t in fn(KB))


def _mfma(fn):
    return tuple(t for KPT in (4, 8) for t in fn(KPT))


def _grid24_replicas(tri):
    t = "true" if tri else "false"
    return _both_kb(lambda KB: (
        _thin(KB, 16, 0, 1, t, 0), _thin(KB, 8, 2, 1, t, 1), _thin(KB, 4, 2, 1, t, 3), _thin(KB, 12, 2, 1, t, 4),
        (f"bwd_thin_kernel<{KB}, 4, 4, {t}>", 0), (f"bwd_thin_kernel<{KB}, 2, 8, {t}>", 1),
        (f"bwd_thin_kernel<{KB}, 1, 8, {t}>", 3), (f"bwd_thin_kernel<{KB}, 4, 4, {t}>", 5),
    )) + _mfma(lambda KPT: ((f"fwd_level_kernel<{KPT}, true, 2, false, false>", 5),)) + (
        ("fwd_wave_kernel<4, 0, 2>", 0), ("fwd_wave_kernel<4, 2, 2>", 1), ("bwd_wave_kernel<4>", 0))


def _grid24_wpf2(tri):
    t = "true" if tri else "false"
    return _both_kb(lambda KB: (_thin(KB, 14, 0, 1, t, 0), _thin(KB, 12, 2, 2, t, 4)))


def _grid24_wpf4(tri):
    t = "true" if tri else "false"
    return _both_kb(lambda KB: (_thin(KB, 12, 0, 1, t, 0), _thin(KB, 12, 2, 4, t, 4))) + _mfma(
        lambda KPT: ((f"bwd_level_kernel<{KPT}, true, false, false>", 0),))


def _grid24_leaf16(tri):
    t = "true" if tri else "false"
    return _both_kb(lambda KB: (_thin(KB, 4, 0, 1, t, 0),))


def _grid40(tri):
    t = "true" if tri else "false"
    return _both_kb(lambda KB: (_thin(KB, 8, 0, 1, t, 0),))


def _star(tri):
    t = "true" if tri else "false"
    return _both_kb(lambda KB: (_thin(KB, 4, 5, 1, t, None), _thin(KB, 8, 5, 1, t, None))) + (
        ("fwd_wave_kernel<4, 5, 2>", None), ("overflow_sum_kernel", None))


CASES = []
for shift in (None, "indefinite"):
    tri = shift is None
    sfx = "" if tri else "_bk"
    CASES += [
        # 1024 copies of a 24 x 24 Q4 grid: 2048 binary fronts of 33-48 own columns on level 4 (one wave per front),
        # 19 456 leaf fronts of up to 64 columns (16 K-steps; backward: >= 1024 fronts, 4 blocks of 16 rows per wave)
        Case("grid24_x1024" + sfx, lambda: grid_matrix(24, 24, 2), shift=shift, replicas=1024,
             targets=_grid24_replicas(tri)),
        # 512 copies, leaves of up to 56 columns: 1024 binary fronts of 33-48 columns (two waves per front), 14 K-steps
        Case("grid24_l56_x512" + sfx, lambda: grid_matrix(24, 24, 2), sym=dict(leaf_size=56), shift=shift,
             replicas=512, targets=_grid24_wpf2(tri)),
        # one copy, leaves of up to 48 columns: two such fronts (four waves per front), 12 K-steps at the leaves
        Case("grid24_l48" + sfx, lambda: grid_matrix(24, 24, 2), sym=dict(leaf_size=48), shift=shift,
             targets=_grid24_wpf4(tri)),
        Case("grid24_l16" + sfx, lambda: grid_matrix(24, 24, 2), sym=dict(leaf_size=16), shift=shift,
             targets=_grid24_leaf16(tri)),
        Case("grid40" + sfx, lambda: grid_matrix(40, 40, 1), sym=dict(leaf_size=24), shift=shift,
             targets=_grid40(tri)),
        # nine grid blocks around a hub: fronts with more than two (and more than kMaxS) children, thin and wave
        Case("star9" + sfx, lambda: star_matrix(9, g=8), sym=dict(leaf_size=32, panel_width=8), shift=shift,
             targets=_star(tri)),
    ]

CASES += [
    # single-tile fronts of 49 own columns under a front with nine children: the tile kernels with surplus planes;
    # the root has several column tiles
    Case("star9_hub40", lambda: star_matrix(9, g=8, hub=40), sym=dict(leaf_size=32, panel_width=8),
         targets=_mfma(lambda KPT: (
             (f"fwd_level_kernel<{KPT}, true, 5, false, false>", 3), (f"bwd_level_kernel<{KPT}, true, false, false>", 3),
             (f"fwd_level_kernel<{KPT}, false, 5, true, false>", 4))) + (
             ("fwd_level_kernel<1, false, 5, false, false>", 4), ("bwd_level_kernel<1, false, false, false>", 4),
             ("bwd_level_kernel<4, false, true, false>", 4), ("bwd_level_kernel<8, false, true, true>", 4))),
    # 3-D Laplacian: multi-tile fronts on binary levels (two-plane level kernels), gathering and pre-assembled
    Case("lap3d16", lambda: lap3d(16), sym=dict(leaf_size=24),
         targets=_mfma(lambda KPT: ((f"fwd_level_kernel<{KPT}, false, 2, true, false>", 8),)) + (
             ("fwd_level_kernel<1, false, 2, false, false>", 8),)),
    Case("lap3d16_pre", lambda: lap3d(16), sym=dict(leaf_size=24), env=(("EIGD_PRE_MIN_WG", "1"),),
         targets=_mfma(lambda KPT: (
             (f"v1_assemble_kernel<{KPT}, 2>", 8), (f"fwd_level_kernel<{KPT}, false, 2, true, true>", 8),
             (f"v1_assemble_kernel<{KPT}, 5>", None), (f"fwd_level_kernel<{KPT}, false, 5, true, true>", None)))),
    # a grid coupled to a hub of 4600 nodes: multi-tile fronts with borders of 4097-7168 rows (index list in LDS)
    Case("hub4600", lambda: hub_matrix(72, 72, 4600, density=0.02), sym=dict(leaf_size=24), reference="schur",
         hub=4600, widths=(16, 32), targets=(("bwd_level_kernel<8, false, true, true>", 6),)),
    # ... of 7300 nodes: borders beyond 7168 rows, the fragment kernel without the index list
    Case("hub7300", lambda: hub_matrix(72, 72, 7300, density=0.02), sym=dict(leaf_size=24), reference="schur",
         hub=7300, widths=(16, 32), targets=(("bwd_level_kernel<8, false, true, false>", 4),)),
]

# the 4 GB edge of the thin forward kernels' 32-bit buffer offsets: n = 65536 rows with ld = 8192 (n * ld * 8 = 2**32)
# takes the tile kernels at the leaves; run by test_thin_buffer_edge, not by the per-case tests
BIG_CASE = Case("grid128x256_ld8192", lambda: grid_matrix(128, 256, 2), widths=(16, 32),
                targets=_mfma(lambda KPT: ((f"fwd_level_kernel<{KPT}, true, 0, false, false>", 0),)))


# conditions (not variants) no case reaches: carry planes of 4 GB or more (v_rows * KB * 8 > kBufMax) send the thin
# levels to the tile kernels as a caller's block beyond 4 GB does (BIG_CASE); it would take a factor of ~17 M rows
NOT_REACHED = ("carry planes of 4 GB or more",)


def all_targets():
    return {v for c in CASES + [BIG_CASE] for v, _ in c.targets}
