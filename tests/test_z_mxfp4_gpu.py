"""OCP MXFP4 linears on the MI355X (tests/mxfp4_cases.py): v_cvt_scalef32_pk_bf16_fp4 held to the restatement weight by weight,
k_gemm_xp / k_gemm_xp_norm WQ = 4 on the matrix cores, the step captured as a graph, and one 7B layer's shapes."""
import pytest

from tests import mxfp4_cases as mx

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_exported_checkpoint_loads_through_from_local(gpu_lib, tmp_path):
    mx.check_exporter_round_trip(gpu_lib, tmp_path, device=DEV)


@pytest.mark.parametrize("max_batch", [16, 32])
def test_one_hot_rows_read_the_dequantised_columns(gpu_lib, max_batch):
    mx.check_one_hot_columns(DEV, gpu_lib, max_batch)


@pytest.mark.parametrize("ksplit", [None, 2, 3])
@pytest.mark.parametrize("max_batch", [16, 32, 64])
def test_every_linear_family_equals_exact_sums(gpu_lib, max_batch, ksplit):
    assert mx.check_linears_exact(DEV, gpu_lib, max_batch, ksplit=ksplit) >= 12 * len(mx.EXACT_ROWS[max_batch])


@pytest.mark.parametrize("B", [3, 40])
@pytest.mark.parametrize("kind", ["moshi", "stt"])
def test_network_vs_the_bf16_oracle_on_the_dequantised_weights(gpu_lib, kind, B):
    mx.check_network_vs_oracle(DEV, gpu_lib, kind, B)


@pytest.mark.parametrize("B", [3, 40])
def test_repeat_streams_are_bit_identical(gpu_lib, B):
    mx.check_repeat_streams(DEV, gpu_lib, B, repeats=2)


def test_refusals(gpu_lib):
    mx.check_refusals(DEV, gpu_lib)


def test_bf16_int8_and_fp8_handles_do_not_notice_an_mxfp4_handle(gpu_lib):
    mx.check_other_classes_do_not_notice(DEV, gpu_lib)


def test_one_7b_layer_shapes_equal_exact_sums(gpu_lib):
    mx.check_7b_layer_shapes(DEV, gpu_lib)
