"""k_sample on the CPU kernel simulator, token for token on crafted logit rows (tests/sampler_cases.py).  The simulator's
mmi_fast_logf is libm's logf; the select, the plateau split, the Philox indexing and the draw are the product's code."""
import pytest

from tests import sampler_cases as sc

# V = 32000 takes the <1024, 32> instantiation.  Measured on the simulator, one process: the whole file 122 s (82 cases), the
# slowest 32000-entry case 3.9 s - affordable, so the simulator runs all four vocabularies like the GPU file
VOCABS = sc.VOCABS


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("k", sc.KS)
def test_fast_path_matches_the_float64_reference_on_crafted_rows(sim_lib, V, k):
    sc.check_crafted("cpu", sim_lib, V, k, "a")


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("k", sc.KS)
def test_supplied_noise_path_matches_the_oracle_on_crafted_rows(sim_lib, V, k):
    sc.check_crafted("cpu", sim_lib, V, k, "b")


@pytest.mark.parametrize("V", VOCABS)
def test_full_multinomial_matches_its_rule_on_crafted_rows(sim_lib, V):
    sc.check_crafted("cpu", sim_lib, V, 25, "c")


@pytest.mark.parametrize("V", VOCABS)
def test_greedy_takes_the_first_maximum_of_crafted_rows(sim_lib, V):
    sc.check_crafted("cpu", sim_lib, V, 25, "d")


@pytest.mark.parametrize("which", ["hi", "lo"])
@pytest.mark.parametrize("mode", ["a", "c"])
@pytest.mark.parametrize("V", VOCABS)
def test_the_largest_and_the_smallest_draw_decide_as_the_reference_says(sim_lib, V, mode, which):
    sc.check_extreme_draw("cpu", sim_lib, V, mode, which)


@pytest.mark.parametrize("mode", ["a", "c"])
@pytest.mark.parametrize("V", VOCABS)
def test_an_all_ones_philox_word_does_not_make_u_one(sim_lib, V, mode):
    sc.check_u_is_never_one("cpu", sim_lib, V, mode)


@pytest.mark.parametrize("V", [2048, 32000])
def test_fast_path_repeats_bit_for_bit_on_fresh_streams(sim_lib, V):
    sc.check_repeat_streams("cpu", sim_lib, V)


def test_the_tie_rule_refuses_at_most_two_percent_of_the_crafted_rows(capsys):
    rate = sc.check_drop_rate()
    with capsys.disabled():
        print(f" [tie rule: {100 * rate:.2f} % of the rows regenerated] ", end="")
