"""The tables of tests/train_kernel_cases.py run on the SIMT emulator (tests/simt), so that the checks of
tests/test_train_kernels_gpu.py guard the training-step kernels without a GPU too.  Every case of every table runs here but one: the
grid-stride PReLU case (T.PRELU_BIG: more than 4096 x 256 units, 4.2 million elements per tensor) is too large for the emulator and runs
on the device only.  Also here, because they need no kernel: the pin of the restated bilinear index arithmetic and the check that plain
torch float32 meets the bounds derived from it (the MEASURED table)."""
import pytest
import torch

import train_kernel_cases as T


@pytest.fixture(scope="module")
def cpu(emu):
    return torch.device("cpu")


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounded"])
@pytest.mark.parametrize("dt,C,entry,pad", T.GATHER_CASES, ids=T.ids(T.GATHER_CASES))
def test_gather_sum_rows_on_the_emulator(cpu, dt, C, entry, pad, exact):
    T.run_gather_sum(cpu, dt, C, entry, pad, exact)


@pytest.mark.parametrize("dt,shape,idt,nan", T.SAMPLE_CASES, ids=T.ids(T.SAMPLE_CASES))
def test_random_sample_rows_bwd_on_the_emulator(cpu, dt, shape, idt, nan):
    T.run_random_sample(cpu, dt, shape, idt, nan)


@pytest.mark.parametrize("dt,K,C,sliced", T.POOL_CASES, ids=T.ids(T.POOL_CASES))
def test_att_pool_rows_on_the_emulator(cpu, dt, K, C, sliced):
    T.run_att_pool(cpu, dt, K, C, sliced)


@pytest.mark.parametrize("dt,C,scale,gk", T.LSM_CASES, ids=T.ids(T.LSM_CASES))
def test_log_softmax_rows_on_the_emulator(cpu, dt, C, scale, gk):
    T.run_log_softmax(cpu, dt, C, scale, gk)


@pytest.mark.parametrize("dt,C,poison", T.LSM_ISOLATION, ids=T.ids(T.LSM_ISOLATION))
def test_log_softmax_rows_keep_a_poisoned_row_to_itself_on_the_emulator(cpu, dt, C, poison):
    T.run_log_softmax_isolation(cpu, dt, C, poison)


@pytest.mark.parametrize("dt,IH,IW,OH,OW,C,exact,native", T.BILINEAR_PARAMS, ids=T.ids(T.BILINEAR_PARAMS))
def test_bilinear_bwd_pm_on_the_emulator(cpu, dt, IH, IW, OH, OW, C, exact, native):
    T.run_bilinear(cpu, dt, IH, IW, OH, OW, C, exact, native)


@pytest.mark.parametrize("dt,shape,fmt,slope,kind", T.PRELU_CASES, ids=T.ids(T.PRELU_CASES))
def test_prelu_on_the_emulator(cpu, dt, shape, fmt, slope, kind):
    T.run_prelu(cpu, dt, shape, fmt, slope, kind)


@pytest.mark.parametrize("B,C,M,U,idt", T.NEAREST_CASES, ids=T.ids(T.NEAREST_CASES))
def test_nearest_interpolation_bwd_channel_major_on_the_emulator(cpu, B, C, M, U, idt):
    T.run_nearest_cm(cpu, B, C, M, U, idt)


def test_restated_bilinear_index_arithmetic_matches_float64_interpolate():
    T.check_bilinear_restatement()


def test_torch_float32_meets_the_bounds_derived_from_it():
    """MEASURED: c = 4 x the recorded ratio of torch float32, and torch float32 on this CPU (its expf may differ from the one the table was
    recorded with) stays within c"""
    for key, r in T.torch_fp32_ratios().items():
        recorded, c = T.MEASURED[key]
        assert c == pytest.approx(4 * recorded, abs=1e-9) and r <= c, (key, r, recorded, c)
