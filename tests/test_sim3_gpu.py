"""orbhip_sim3_iterate on the MI355X against tests/sim3_model.py: the cases and checks of tests/test_sim3_emu.py (tests/sim3_checks.py) on the real
library.  Horn is compared with the recorded tolerance; everything after it must follow exactly from the kernel's own R, t, s."""
import pytest

import sim3_cases as Cs
import sim3_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", Cs.ALL_NAMES)
def test_kernel_equals_model(gpu_lib, name):
    K.check_case(name, gpu_lib, exact=False)


def test_threshold_is_truncated_to_an_integer(gpu_lib):
    K.check_threshold_is_truncated(gpu_lib)


def test_selection_rules(gpu_lib):
    K.check_select_rules(gpu_lib)


def test_no_best_leaves_the_record_untouched(gpu_lib):
    K.check_untouched_without_best(gpu_lib)


def test_identical_sets_and_collinear_triples(gpu_lib):
    K.check_non_finite(gpu_lib)


def test_refused_inputs(gpu_lib):
    K.check_refused_inputs(gpu_lib)


def test_fewer_than_three_correspondences_touch_nothing(gpu_lib):
    K.check_short_untouched(gpu_lib)


def test_batch_slots_give_the_same_bits(gpu_lib):
    K.check_batch_slots(gpu_lib)


def test_repeated_call_gives_the_same_bits(gpu_lib):
    K.check_repeat(gpu_lib)


def test_three_threads(gpu_lib):
    K.check_three_threads(gpu_lib)


def test_solver_rounds_and_draw_queue(gpu_lib):
    K.check_solver_rounds(gpu_lib, exact=False)


def test_dropin_cpp_equals_the_c_abi(gpu_lib, tmp_path):
    K.run_cpp(K.build_cpp(tmp_path, gpu_lib))
