"""The case tables of tests/pm_cases.py hold what they claim -- no GPU needed: every (form, feature value) pair of the point-major GEMM
family at least once, the "everything at once" case of every form, every case inside its form's domain and every rejected one outside;
and the shapes of the boundary table take the form the table says (ffb6d_mlp_pm_choice is a pure host function)."""
import collections

import pytest

import pm_cases as pc


def test_every_form_meets_every_feature_value():
    count = collections.Counter((c.form, a, v) for c in pc.CASES for a, v in pc.features(c).items())
    missing = [(form, a, v) for form in pc.FORMS for a, v in pc.required(form) if count[(form, a, v)] == 0]
    assert not missing, missing


def _pairs(cases):
    out = set()
    for c in cases:
        f = pc.features(c)
        out |= {(c.form, a, f[a], b, f[b]) for a in pc.FEATURE_AXES for b in pc.FEATURE_AXES if a < b and a in f and b in f}
    return out


def test_every_pair_of_feature_values_is_in_the_table():
    """src2 x x1_gather, epi x in_slice, hint x bits, sched x out_slice ...: every pair of values that the 400 draws per dtype from a
    form's domain come up with is held by a case of the table"""
    for form in pc.FORMS:
        missing = _pairs(pc.candidates(form)[1]) - _pairs(c for c in pc.CASES if c.form == form)
        assert not missing, sorted(missing)[:10]


def test_everything_at_once_per_form_and_plan():
    for form in pc.FORMS:
        for dt in pc.DTYPES[form]:
            for h in pc.HINTS[form]:
                assert any(pc.is_everything(c) for c in pc.CASES if (c.form, c.dt, c.hint) == (form, dt, h)), (form, dt, h)


def test_cases_lie_inside_the_domain_and_rejected_ones_outside():
    assert all(pc.in_domain(c) for c in pc.CASES)
    assert not any(pc.in_domain(c) for _, c in pc.REJECTED)
    assert {c.form for _, c in pc.REJECTED} >= {"stream", "lds", "seq", "big"}
    for c in pc.CASES:
        assert (c.P in pc.ROWS or (c.form == "seq" and c.P == pc.SEQ_ROWS)) and c.B in pc.FRAMES and c.K1 + c.K2 <= 256 and c.cout <= 528
        assert c.cout > 3 or c.form in ("t1", "t2", "t3", "t4", "t5")
        assert (c.dt == "f32") == (c.form == "seq") or c.form not in ("seq", "big")


def test_table_is_deterministic():
    assert pc._table() == pc.CASES
    assert len({pc.case_id(c) for c in pc.CASES}) == len(pc.CASES)


def test_batched_and_lfa_tables_hold_every_value():
    assert {b[0] for b in pc.BATCHED} == {1, 2, 16, 36} and {b[1] for b in pc.BATCHED} == {128, 384}
    assert {b[2] for b in pc.BATCHED} == {128, 160, 256} and {b[4] for b in pc.BATCHED} == set(pc.BATCHED_HINTS)
    assert all(b[3] % 4 == 0 for b in pc.BATCHED) and any(b[3] % 128 for b in pc.BATCHED)
    assert {(G, h) for G, _, _, _, h in pc.BATCHED} == {(G, h) for G in (1, 2, 16, 36) for h in pc.BATCHED_HINTS}
    for col, vals in ((2, pc.LFA_N), (3, (1, 2)), (4, (32, 64))):
        for key in (0, 1):                       # every d, and every p_hint, with every N, mode and index type
            for k in (pc.LFA_D, pc.LFA_HINT)[key]:
                assert {c[col] for c in pc.LFA if (c[key] & 255 if key else c[key]) == k} == set(vals), (key, k, col)
    assert {(c[0], c[1] & 255) for c in pc.LFA} == {(d, h) for d in pc.LFA_D for h in pc.LFA_HINT}


@pytest.mark.parametrize("what,rows,cout,k1,k2,act,bf16,xg,form", pc.BOUNDARIES)
def test_automatic_choice_takes_the_form_the_boundary_table_says(native_lib, what, rows, cout, k1, k2, act, bf16, xg, form):
    assert native_lib.ffb6d_mlp_pm_choice(rows, cout, k1, k2, act, bf16, xg) & 255 == form


def test_boundary_table_reaches_every_form_and_the_fallbacks_start_from_theirs(native_lib):
    forms = collections.Counter(b[-1] for b in pc.BOUNDARIES)
    assert set(forms) == {1, 2, 3, 4, 5, 6, 7, 8, 9}
    for what, rows, cout, k1, bf16, form, extra in pc.FALLBACKS:
        assert native_lib.ffb6d_mlp_pm_choice(rows, cout, k1, 0, 1, bf16, 0) & 255 == form and extra % (8 if bf16 else 4)
