"""orbhip_pose_optimization on the MI355X against tests/pose_opt_model.py: the cases and checks of tests/test_pose_opt_emu.py (tests/pose_opt_checks.py)
on the real library."""
import pytest

import pose_opt_cases as Cs
import pose_opt_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", Cs.ALL_NAMES)
def test_kernel_equals_model(gpu_lib, name):
    K.check_case(name, gpu_lib)


def test_repeated_call_gives_the_same_bits(gpu_lib):
    K.check_repeat(gpu_lib)


def test_batch_slots_give_the_same_bits(gpu_lib):
    K.check_batch_slots(gpu_lib)


def test_batch_of_size_and_degenerate_cases(gpu_lib):
    K.check_batch_edges(gpu_lib)


def test_frame_form_equals_host_array_form(gpu_lib):
    K.check_frame_form(gpu_lib)


def test_fewer_than_three_observations_touch_nothing(gpu_lib):
    K.check_short_untouched(gpu_lib)


def test_three_threads(gpu_lib):
    K.check_three_threads(gpu_lib)


def test_dropin_cpp_equals_the_c_abi(gpu_lib, tmp_path):
    K.run_cpp(K.build_cpp(tmp_path, gpu_lib))
