"""The sweep catalog (tests/sweep_catalog.py) against the library's table of launch variants -- host only."""


def test_sweep_catalog_covers_every_variant():
    """every variant the compiled sweeps can launch is a target of some catalog case or excluded with a reason, and
    nothing else is named: a launch-policy change that adds or removes a variant fails here until the catalog follows"""
    from eigd_amd.device import sweep_variants
    from sweep_catalog import EXCLUDED, all_targets

    table = sweep_variants()
    assert len(table) == len(set(table))
    targets = all_targets()
    assert not (targets & set(EXCLUDED)), sorted(targets & set(EXCLUDED))
    assert all(reason.strip() for reason in EXCLUDED.values())
    missing = set(table) - targets - set(EXCLUDED)
    unknown = (targets | set(EXCLUDED)) - set(table)
    assert not missing, f"variants no catalog case launches: {sorted(missing)}"
    assert not unknown, f"catalog names variants the library does not have: {sorted(unknown)}"


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
