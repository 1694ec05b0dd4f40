"""orbhip_sim3_optimize on the MI355X against tests/sim3_opt_model.py: the cases and checks of tests/test_sim3_opt_emu.py (tests/sim3_opt_checks.py)
on the real library."""
import pytest

import sim3_opt_cases as Cs
import sim3_opt_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", Cs.ALL_NAMES)
def test_kernel_equals_model(gpu_lib, name):
    K.check_case(name, gpu_lib)


def test_repeated_call_gives_the_same_bits(gpu_lib):
    K.check_repeat(gpu_lib)


def test_batch_slots_give_the_same_bits(gpu_lib):
    K.check_batch_slots(gpu_lib)


def test_no_pairs_touch_nothing_and_bad_arguments_are_refused(gpu_lib):
    K.check_empty_and_bad_arguments(gpu_lib)


def test_three_threads(gpu_lib):
    K.check_three_threads(gpu_lib)


def test_dropin_cpp_equals_the_c_abi(gpu_lib, tmp_path):
    K.run_cpp(K.build_cpp(tmp_path, gpu_lib))
