"""orbhip_sim3_iterate (orb_slam2_amd/csrc/orbhip_sim3.hip) under CPU emulation against tests/sim3_model.py: every graded case of tests/sim3_cases.py
(sizes around the wave, 1, 5 and 300 hypotheses, fixed and free scale, both gemm modes), where the emulated kernel must give the model's bits end to end;
the dedicated cases, batch slots, repeatability, threads, the class's loop and the C++ drop-in (also under AddressSanitizer and UBSan as a stand-alone
program).  The checks themselves are in tests/sim3_checks.py, shared with the device run (tests/test_sim3_gpu.py)."""
import os

import pytest

import sim3_cases as Cs
import sim3_checks as K


@pytest.mark.parametrize("name", Cs.ALL_NAMES)
def test_kernel_equals_model(emu_lib, name):
    K.check_case(name, emu_lib, exact=True)


def test_generator_rejects_few_triples():
    K.check_rejected_share()


def test_threshold_is_truncated_to_an_integer(emu_lib):
    K.check_threshold_is_truncated(emu_lib)


def test_selection_rules(emu_lib):
    K.check_select_rules(emu_lib)


def test_no_best_leaves_the_record_untouched(emu_lib):
    K.check_untouched_without_best(emu_lib)


def test_identical_sets_and_collinear_triples(emu_lib):
    K.check_non_finite(emu_lib)


def test_refused_inputs(emu_lib):
    K.check_refused_inputs(emu_lib)


def test_fewer_than_three_correspondences_touch_nothing(emu_lib):
    K.check_short_untouched(emu_lib)


def test_batch_slots_give_the_same_bits(emu_lib):
    K.check_batch_slots(emu_lib)


def test_repeated_call_gives_the_same_bits(emu_lib):
    K.check_repeat(emu_lib)


def test_three_threads(emu_lib):
    K.check_three_threads(emu_lib)


def test_solver_rounds_and_draw_queue(emu_lib):
    K.check_solver_rounds(emu_lib, exact=True)


def test_dropin_cpp_equals_the_c_abi(emu_lib, tmp_path):
    K.run_cpp(K.build_cpp(tmp_path, emu_lib))


def test_dropin_cpp_under_address_and_undefined_sanitizers(emu_lib, tmp_path):
    """the stand-alone program and the drop-in file built with -fsanitize=address,undefined (the program itself is linked with the sanitizers: nothing
    is preloaded) and run against the emulation library.  The kernels' own file is covered by `make emu_asan` (it is in the Makefile's SRCS)."""
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    env.pop("ASAN_OPTIONS", None)
    K.run_cpp(K.build_cpp(tmp_path, emu_lib, sanitize=True), env=env)
