"""orbhip_pnp_iterate on the MI355X against tests/pnp_model.py: the cases and checks of tests/test_pnp_emu.py (tests/pnp_checks.py) on the real library.
Every record must equal the model's bit for bit: a differing bit on the device is a contraction or a re-associated sum to be found, not a spread."""
import pytest

import pnp_cases as Cs
import pnp_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", Cs.ALL_NAMES)
def test_kernel_equals_model(gpu_lib, name):
    K.check_case(name, gpu_lib)


def test_threshold_is_strict(gpu_lib):
    K.check_strict_threshold(gpu_lib)


def test_selection_rules(gpu_lib):
    K.check_select_rules(gpu_lib)


def test_carried_in_mask_is_refined_first(gpu_lib):
    K.check_carried_in(gpu_lib)


def test_point_behind_the_camera_is_judged_by_the_arithmetic(gpu_lib):
    K.check_behind_camera(gpu_lib)


def test_coincident_and_collinear_sets(gpu_lib):
    K.check_degenerate(gpu_lib)


def test_refused_inputs(gpu_lib):
    K.check_refused_inputs(gpu_lib)


def test_short_problems_touch_nothing(gpu_lib):
    K.check_short_untouched(gpu_lib)


def test_batch_slots_give_the_same_bits(gpu_lib):
    K.check_batch_slots(gpu_lib)


@pytest.mark.parametrize("name", Cs.REFINE_NAMES)
def test_refine_equals_model(gpu_lib, name):
    K.check_refine_case(name, gpu_lib)


def test_sign_rule_reads_the_first_set_bit(gpu_lib):
    K.check_sign_first(gpu_lib)


@pytest.mark.parametrize("name", K.PASS_SEQUENCES)
def test_selection_across_passes(gpu_lib, name):
    K.check_select_passes(name, gpu_lib)


def test_fewer_refine_rows_than_refines(gpu_lib):
    K.check_ref_cap(gpu_lib)


def test_hypothesis_counts_alone(gpu_lib):
    K.check_hyp_count_alone(gpu_lib)


def test_batch_of_refining_problems(gpu_lib):
    K.check_batch_refines(gpu_lib)


def test_repeated_call_gives_the_same_bits(gpu_lib):
    K.check_repeat(gpu_lib)


def test_three_threads(gpu_lib):
    K.check_three_threads(gpu_lib)


def test_solver_rounds_and_draw_queue(gpu_lib):
    K.check_solver_rounds(gpu_lib)


def test_dropin_cpp_equals_the_c_abi(gpu_lib, tmp_path):
    """as under emulation, and one call of 4100 hypotheses, which the class cuts at 4096 with the best count and mask carried over"""
    K.run_cpp(K.build_cpp(tmp_path, gpu_lib), split=True)
