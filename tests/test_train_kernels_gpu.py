"""The training step's hand-written kernels (csrc/train_rows.hip, csrc/train_ops.hip, the privatised scatter of
csrc/neighbour_ops.hip) held to float64: exact-integer cases compared bit for bit, rounded cases within half an ulp of the output type
plus a derived number of float32 roundings.  Tables, references and bounds: tests/train_kernel_cases.py.  Every operator is driven through
its public Python entry and the log of native entry points shows that the kernel ran.  Runs under --emulate too; the grid-stride PReLU
case (4.2 million elements) is the one to deselect there, as tests/test_train_kernels_emu_cpu.py does, which runs the same tables on the
emulator as part of the CPU suite."""
import pytest

import train_kernel_cases as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounded"])
@pytest.mark.parametrize("dt,C,entry,pad", T.GATHER_CASES, ids=T.ids(T.GATHER_CASES))
def test_gather_sum_rows(device, dt, C, entry, pad, exact):
    T.run_gather_sum(device, dt, C, entry, pad, exact)


@pytest.mark.parametrize("dt,shape,idt,nan", T.SAMPLE_CASES, ids=T.ids(T.SAMPLE_CASES))
def test_random_sample_rows_bwd(device, dt, shape, idt, nan):
    T.run_random_sample(device, dt, shape, idt, nan)


@pytest.mark.parametrize("dt,K,C,sliced", T.POOL_CASES, ids=T.ids(T.POOL_CASES))
def test_att_pool_rows(device, dt, K, C, sliced):
    T.run_att_pool(device, dt, K, C, sliced)


@pytest.mark.parametrize("dt,C,scale,gk", T.LSM_CASES, ids=T.ids(T.LSM_CASES))
def test_log_softmax_rows(device, dt, C, scale, gk):
    T.run_log_softmax(device, dt, C, scale, gk)


@pytest.mark.parametrize("dt,C,poison", T.LSM_ISOLATION, ids=T.ids(T.LSM_ISOLATION))
def test_log_softmax_rows_keep_a_poisoned_row_to_itself(device, dt, C, poison):
    T.run_log_softmax_isolation(device, dt, C, poison)


@pytest.mark.parametrize("dt,IH,IW,OH,OW,C,exact,native", T.BILINEAR_PARAMS, ids=T.ids(T.BILINEAR_PARAMS))
def test_bilinear_bwd_pm(device, dt, IH, IW, OH, OW, C, exact, native):
    T.run_bilinear(device, dt, IH, IW, OH, OW, C, exact, native)


@pytest.mark.parametrize("dt,shape,fmt,slope,kind", T.PRELU_CASES, ids=T.ids(T.PRELU_CASES))
def test_prelu(device, dt, shape, fmt, slope, kind):
    T.run_prelu(device, dt, shape, fmt, slope, kind)


@pytest.mark.parametrize("dt,shape,fmt", T.PRELU_BIG, ids=T.ids(T.PRELU_BIG))
def test_prelu_grid_stride_loop(device, dt, shape, fmt):
    """more units than 4096 workgroups of 256 threads; all four slopes"""
    for slope in T.SLOPES:
        T.run_prelu(device, dt, shape, fmt, slope, "big")


@pytest.mark.parametrize("B,C,M,U,idt", T.NEAREST_CASES, ids=T.ids(T.NEAREST_CASES))
def test_nearest_interpolation_bwd_channel_major(device, B, C, M, U, idt):
    T.run_nearest_cm(device, B, C, M, U, idt)
