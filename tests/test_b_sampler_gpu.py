"""k_sample on a real MI355X, token for token on crafted logit rows (tests/sampler_cases.py): the three instantiations, the
hardware logarithm, every mode of the sampler; and lm_cases.check_topk_device_rng - the token-for-token check of the production
path on the model's own logits, audio sites with the fused next-input write included - which so far ran on the simulator only."""
import pytest

from moshi_amd.config import LMConfig
from tests import lm_cases
from tests import sampler_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("V", sc.VOCABS)
@pytest.mark.parametrize("k", sc.KS)
def test_fast_path_matches_the_float64_reference_on_crafted_rows(gpu_lib, V, k):
    sc.check_crafted(DEV, None, V, k, "a")


@pytest.mark.parametrize("V", sc.VOCABS)
@pytest.mark.parametrize("k", sc.KS)
def test_supplied_noise_path_matches_the_oracle_on_crafted_rows(gpu_lib, V, k):
    sc.check_crafted(DEV, None, V, k, "b")


@pytest.mark.parametrize("V", sc.VOCABS)
def test_full_multinomial_matches_its_rule_on_crafted_rows(gpu_lib, V):
    sc.check_crafted(DEV, None, V, 25, "c")


@pytest.mark.parametrize("V", sc.VOCABS)
def test_greedy_takes_the_first_maximum_of_crafted_rows(gpu_lib, V):
    sc.check_crafted(DEV, None, V, 25, "d")


@pytest.mark.parametrize("which", ["hi", "lo"])
@pytest.mark.parametrize("mode", ["a", "c"])
@pytest.mark.parametrize("V", sc.VOCABS)
def test_the_largest_and_the_smallest_draw_decide_as_the_reference_says(gpu_lib, V, mode, which):
    sc.check_extreme_draw(DEV, None, V, mode, which)


@pytest.mark.parametrize("mode", ["a", "c"])
@pytest.mark.parametrize("V", sc.VOCABS)
def test_an_all_ones_philox_word_does_not_make_u_one(gpu_lib, V, mode):
    sc.check_u_is_never_one(DEV, None, V, mode)


@pytest.mark.parametrize("V", sc.VOCABS)
def test_fast_path_repeats_bit_for_bit_on_fresh_streams(gpu_lib, V):
    sc.check_repeat_streams(DEV, None, V)


def test_production_sampler_token_for_token_tiny(gpu_lib):
    lm_cases.check_topk_device_rng(DEV, None)


def test_production_sampler_token_for_token_full_vocabularies(gpu_lib):
    """32000 text / 2048 audio entries, top-k 25 / 250: the audio sites are k_sample<256, 8, true> with the fused next-input write."""
    lm_cases.check_topk_device_rng(DEV, None, LMConfig(num_layers=1, context=16), top_k=250, top_k_text=25)
