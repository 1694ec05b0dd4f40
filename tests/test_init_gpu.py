"""orbhip_init_reconstruct on the MI355X against tests/init_model.py: the cases and checks of tests/test_init_emu.py (tests/init_checks.py) on the real
library.  Every record must equal the model's bit for bit: a differing bit on the device is a contraction or a re-associated sum to be found, not a
spread."""
import pytest

import init_cases as Cs
import init_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", Cs.ALL_NAMES)
def test_kernel_equals_model(gpu_lib, name):
    K.check_case(name, gpu_lib)


def test_chi_square_thresholds_are_strict(gpu_lib):
    K.check_strict_thresholds(gpu_lib)


def test_reprojection_threshold_is_strict(gpu_lib):
    K.check_strict_reprojection(gpu_lib)


def test_non_finite_triangulation_is_skipped(gpu_lib):
    K.check_non_finite_triangulation_is_skipped(gpu_lib)


def test_tie_of_two_best_scores_keeps_the_first(gpu_lib):
    K.check_tie_keeps_first(gpu_lib)


def test_equal_smallest_eigenvalues_keep_the_first(gpu_lib):
    K.check_equal_smallest_eigenvalues_keep_the_first(gpu_lib)


def test_all_scores_zero_returns_false_without_a_model(gpu_lib):
    K.check_all_scores_zero(gpu_lib)


def test_similar_rule_is_strict_at_zero(gpu_lib):
    K.check_similar_rule_is_strict(gpu_lib)


def test_point_without_parallax_is_counted_not_triangulated(gpu_lib):
    K.check_low_parallax_point_is_kept(gpu_lib)


def test_non_finite_coordinates(gpu_lib):
    K.check_non_finite(gpu_lib)


def test_refused_inputs(gpu_lib):
    K.check_refused_inputs(gpu_lib)


def test_batch_slots_give_the_same_bits(gpu_lib):
    K.check_batch_slots(gpu_lib)


def test_without_optional_outputs(gpu_lib):
    K.check_without_optional_outputs(gpu_lib)


def test_repeated_call_gives_the_same_bits(gpu_lib):
    K.check_repeat(gpu_lib)


def test_three_threads(gpu_lib):
    K.check_three_threads(gpu_lib)


def test_dropin_cpp_equals_the_c_abi(gpu_lib, tmp_path):
    """as under emulation; rand() is the process's, and in this process the device runtime runs between the calls: the first call's sets must be the
    generator's from seed 0 and no later call may start again (the whole stream is asserted under emulation)"""
    K.run_cpp(K.build_cpp(tmp_path, gpu_lib), gpu_lib, tmp_path, whole_stream=False)
