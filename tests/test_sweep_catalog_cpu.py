"""The sweep catalog (tests/sweep_catalog.py) against the library's table of launch variants and against its launch
policy -- host only."""
import pytest

from sweep_catalog import BIG_CASE, CASES, matrix_of


def test_sweep_catalog_covers_every_variant():
    """every variant the library compiles is a target of some catalog case, and nothing else is named: a launch-policy
    change that adds or removes a variant fails here until the catalog follows"""
    from eigd_amd.device import sweep_variants
    from sweep_catalog import all_targets

    table = sweep_variants()
    assert len(table) == len(set(table))
    targets = all_targets()
    missing = set(table) - targets
    unknown = targets - set(table)
    assert not missing, f"variants no catalog case launches: {sorted(missing)}"
    assert not unknown, f"catalog names variants the library does not have: {sorted(unknown)}"


@pytest.mark.parametrize("case", CASES + [BIG_CASE], ids=[c.name for c in CASES + [BIG_CASE]])
def test_planned_launches_hold_every_target(case, monkeypatch):
    """
    The launch policy, asked on the host (Symbolic.sweep_plan), plans every (variant, level) target of the case for the
    symbolic analysis the GPU test factors (level None: at any level).  All 18 cases run, the two of 1 179 648 rows
    (grid24_x1024, grid24_x1024_bk) included: 10.5 s together on one core, of which those two take 4.4 s.  BIG_CASE's
    targets are those of a caller's block beyond 4 GB: thin_buf = False, no buffer needed.
    """
    from eigd_amd.device import Symbolic, sweep_variants

    for name, value in case.env:
        monkeypatch.setenv(name, value)
    A, _, _ = matrix_of(case)
    sym = Symbolic(A, **case.sym)
    table = set(sweep_variants())
    planned = set()
    for w in case.widths:
        plan = sym.sweep_plan(w, tri=case.shift is None, thin_buf=case is not BIG_CASE)
        assert plan and {v for v, _ in plan} <= table
        assert all(0 <= lvl < sym.sizes["nlevels"] for _, lvl in plan)
        planned |= set(plan)
    names = {v for v, _ in planned}
    missing = [(v, lvl) for v, lvl in case.targets if (v not in names if lvl is None else (v, lvl) not in planned)]
    assert not missing, f"{case.name}: not planned {missing}; planned {sorted(planned)}"


def test_sweep_plan_follows_its_inputs():
    """width classes (4 / 16 / 32 columns), tri and thin_buf select the kernels; EIGD_PRE_MIN_WG is read per query"""
    from eigd_amd.device import Symbolic

    A, _, _ = matrix_of(BIG_CASE)
    sym = Symbolic(A)
    assert sym.sweep_plan(5) == sym.sweep_plan(16) != sym.sweep_plan(17)
    assert sym.sweep_plan(1) == sym.sweep_plan(4) != sym.sweep_plan(5)
    thin = [v for v, _ in sym.sweep_plan(32) if v.startswith("fwd_thin_kernel<32,")]
    assert thin and all(v.endswith(", true>") for v in thin)
    assert [v for v, _ in sym.sweep_plan(32, tri=False)] == [
        v.replace(", true>", ", false>") if "_thin_" in v else v for v, _ in sym.sweep_plan(32)]
    assert not [v for v, _ in sym.sweep_plan(32, thin_buf=False) if v.startswith("fwd_thin_kernel")]
    with pytest.raises(Exception, match="columns"):
        sym.sweep_plan(33)


def test_sweep_catalog_cases_are_well_formed():
    from sweep_catalog import BIG_CASE, CASES, KB_OF_KPT

    names = [c.name for c in CASES]
    assert len(names) == len(set(names))
    for c in CASES + [BIG_CASE]:
        assert c.targets and c.shift in (None, "indefinite") and c.reference in ("splu", "schur")
        assert set(c.widths) <= set(KB_OF_KPT.values())
        for v, lvl in c.targets:
            kb = int(v.split("<")[1].split(",")[0].rstrip(">")) if "<" in v else None
            if v.startswith(("fwd_thin", "bwd_thin", "fwd_wave", "bwd_wave")):
                assert kb in c.widths, (c.name, v)           # the sweep width that launches it is solved
            elif v.startswith(("fwd_level", "bwd_level", "v1_assemble")):
                assert KB_OF_KPT[kb] in c.widths, (c.name, v)
