"""The references of the rigid-fit tests pin themselves, and the kernel source runs against them without a GPU.

1. fit64 (float64, LAPACK SVD: the reference's own best_fit_transform) against fit_ld (the same fit in np.longdouble by a
   one-sided Jacobi) on EVERY case of tests/rigid_fit_cases.py -- 16 200 point sets of 1, 2, 3, 4, 9 and 50 points.  Measured:

       largest |R64 - R_ld| / cond                          9.2e-15     (over the 9815 cases with cond <= 1e10)
       largest (objective(R64) - objective(R_ld)) / s1      3.4e-15

   (both on the sets with s1 = s2 = s3, where cond = 1/2; the thin families measure 2e-16 .. 5e-16 and 1e-16 .. 1e-15).

   These two numbers, which no kernel had a part in, are rigid_fit_cases.REF_ROT and REF_OBJ, and the bars of the device tests
   are ten times them (the margin is for the other summation order of H and for the kernel's fixed sweep schedule):

       ROT_BAR = 9.2e-14:   |R_dev - R64| <= ROT_BAR * cond       wherever cond <= 1e10
       OBJ_BAR = 3.4e-14:   objective(R_dev) - objective(R64) <= OBJ_BAR * s1        for every case

   The test prints both figures and fails if they are not reproduced within a factor 1.5 either way.

2. The assertions of tests/test_rigid_fit_gpu.py through the unmodified kernel sources on the SIMT emulator of tests/simt:
   best_fit_transform_batch (csrc/pose.hip) bound as in tests/test_simt_stages_cpu.py, and one ICP iteration (csrc/icp.hip)
   through the C ABI as in tests/test_refine_emu_cpu.py.

With the decomposition this file was written against (Jacobi eigenvectors of H^T H) part 2 failed in about 950 of the 2500
rotation cases of every n >= 3, 210 to 280 objective cases, the permutation test and the ICP test.  Largest |R - R64| / cond on
the emulator then, against the bar of 9.2e-14 (n = 50; largest |R - R64| itself: 1.7):
    strip 1:1e-2:0  6.9e-13     strip 1:1e-3:0  1.6e-10     strip 1:1e-4:0  7.0e-9      line + noise / rounding  2.4e-9
    rod 1:1e-2:1e-2 3.3e-13     rod 1:1e-3:1e-3 4.7e-11     rod 1:1e-4:1e-4 3.3e-9
and with three points also planar 1.1e-12, strip 1:1e-1:0 9.3e-12, rod 1:1e-1:1e-1 5.0e-13; excess objective / s1 up to 1.1e-8
(strips and rods of 1e-3 and thinner, lines), bar 3.4e-14; ICP update on centred clouds: strip 1e-3 2.2e-11, strip 1e-4 1.6e-9,
rod 1e-3 9.0e-12, rod 1e-4 4.1e-10.  Full-bodied sets and the cube passed (4e-15 .. 9e-15).  With the one-sided Jacobi on H
every family is at or below the reference's own figure (largest 9.2e-15 and 5.7e-15).
"""
import numpy as np
import pytest
import torch

import rigid_fit_cases as C
import test_rigid_fit_gpu as TG
from test_refine_emu_cpu import _p, emu_icp, prepare      # noqa: F401  (emu_icp is a fixture)

CPU = torch.device("cpu")


def test_case_table_is_complete_and_classified():
    total = 0
    for n in C.NS:
        A, B, meta = C.build(n)
        total += len(A)
        assert A.dtype == B.dtype == np.float32 and A.shape == B.shape == (len(meta), n, 3)
        assert len(A) > 64 and len(A) % 64 != 0
        assert np.isfinite(A).all() and np.isfinite(B).all()
        cond = C.reference(n)["cond"]
        assert not ((cond >= C.COND_BAND[0]) & (cond <= C.COND_BAND[1])).any()
        sel = TG.rot_class(n)                                    # raises on a case of neither class
        fam = {m["family"] for m in meta}
        assert {"full", "planar", "line", "equal"} <= fam and all(f"rod{t:g}" in fam and f"strip{t:g}" in fam for t in C.TAUS)
        if n >= 3:                                               # every family that can fix a rotation does so somewhere ...
            for f in fam - {"equal"}:
                assert any(s for s, m in zip(sel, meta) if m["family"] == f), f
        if n >= 4:                                               # ... and the thin ones reach far: cond 1e7 and beyond
            assert cond[sel].max() > 1e9 and any(m["family"] == "cube" and m["mirror"] and not s for s, m in zip(sel, meta))
        else:
            assert n > 2 or not sel.any()
    assert total == 16200
    A, B, _ = C.build(9)
    A2, B2, _ = C.build.__wrapped__(9)                           # deterministic
    assert np.array_equal(A, A2) and np.array_equal(B, B2)


def test_reference_against_extended_precision():
    rot, obj = 0.0, 0.0
    for n in C.NS:
        A, B, meta = C.build(n)
        ref, ld = C.reference(n), C.fit_ld(A, B)
        sel = ref["cond"] <= C.COND_MAX
        s1 = ld["s"][:, 0]
        # the two decompositions agree on what they decompose
        assert np.all(np.abs(ref["s"] - ld["s"].astype(np.float64)) <= 1e-14 * ref["s"][:, :1])
        orth = np.abs((np.swapaxes(ld["R"], 1, 2) @ ld["R"]).astype(np.float64) - np.eye(3)).max()
        assert orth < 1e-17, orth
        err = np.abs(ref["R"] - ld["R"]).max(axis=(1, 2)).astype(np.float64)
        ratio = np.where(sel, err / np.where(sel, ref["cond"], 1), 0)
        excess = ref["obj"] - C.objective(ld["R"], A, B)
        pos = s1 > 0
        assert np.all(excess[~pos] == 0)
        rel = np.where(pos, excess / np.where(pos, s1, 1), 0).astype(np.float64)
        print(f"n={n}: |R64 - R_ld| / cond {ratio.max():.3e} {C.by_family(meta, ratio, sel)}")
        print(f"n={n}: excess objective / s1 {rel.max():.3e} {C.by_family(meta, rel, pos)}")
        rot, obj = max(rot, ratio.max()), max(obj, rel.max())
    print(f"fit64 against fit_ld: largest |R64 - R_ld| / cond = {rot:.3e}, largest excess objective / s1 = {obj:.3e}")
    assert C.REF_ROT / 1.5 <= rot <= C.REF_ROT * 1.5 and C.REF_OBJ / 1.5 <= obj <= C.REF_OBJ * 1.5
    assert C.ROT_BAR == 10 * C.REF_ROT and C.OBJ_BAR == 10 * C.REF_OBJ


# ---- the kernel sources on the emulator -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.NS)
def test_fit_on_the_emulator(emu, n):
    TG.test_output_is_a_rigid_transform(CPU, n)
    TG.test_objective_is_the_minimum(CPU, n)
    TG.test_rotation_matches_float64_svd(CPU, n)


def test_fit_properties_on_the_emulator(emu):
    TG.test_zero_covariance_gives_the_identity_exactly(CPU)
    TG.test_a_problem_alone_gives_the_bits_of_the_batch(CPU)
    TG.test_nan_and_inf_problems_leave_their_neighbours_alone(CPU)
    for e in (-20, 20):
        TG.test_scaling_by_a_power_of_two(CPU, e)
    TG.test_permuting_the_points(CPU)


def test_icp_update_on_the_emulator(emu_icp):
    lib = emu_icp

    def run_icp(case, models):
        buf, n_cls, total = prepare(lib, models)
        P, (B, N) = len(case["frame_of"]), case["mask"].shape
        wbytes = lib.ffb6d_icp_workspace_bytes(P, N)
        ws = np.zeros(wbytes, np.uint8)
        T, n_pairs = np.full((P, 3, 4), 7.0), np.full(P, 7, np.int32)
        rms, iters = np.full(P, 7, np.float32), np.full(P, 7, np.int32)
        rc = lib.ffb6d_icp_refine_f32(_p(buf), n_cls, total, _p(case["pcld"]), _p(case["mask"]), 64, None, _p(case["frame_of"]),
                                      _p(case["class_of"]), _p(case["T0"]), P, B, N, N, float("inf"), 1, 0.0, 3, _p(T), _p(n_pairs),
                                      _p(rms), _p(iters), _p(ws), wbytes, None)
        assert rc == 0, lib.ffb6d_last_error()
        return T, n_pairs, iters
    TG.check_icp_one_iteration(run_icp)
