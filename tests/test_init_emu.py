"""orbhip_init_reconstruct (orb_slam2_amd/csrc/orbhip_init.hip) under CPU emulation against tests/init_model.py: every case of tests/init_cases.py,
where the emulated kernels must give the model's bits in every hypothesis record, every motion-hypothesis record and the whole answer; the dedicated
cases, batch slots, repeatability and threads.  The checks themselves are in tests/init_checks.py, shared with the device run
(tests/test_init_gpu.py)."""
import os

import pytest

import init_cases as Cs
import init_checks as K


@pytest.mark.parametrize("name", Cs.ALL_NAMES)
def test_kernel_equals_model(emu_lib, name):
    K.check_case(name, emu_lib)


def test_generator_conditions():
    K.check_conditions()


def test_chi_square_thresholds_are_strict(emu_lib):
    K.check_strict_thresholds(emu_lib)


def test_reprojection_threshold_is_strict(emu_lib):
    K.check_strict_reprojection(emu_lib)


def test_non_finite_triangulation_is_skipped(emu_lib):
    K.check_non_finite_triangulation_is_skipped(emu_lib)


def test_tie_of_two_best_scores_keeps_the_first(emu_lib):
    K.check_tie_keeps_first(emu_lib)


def test_equal_smallest_eigenvalues_keep_the_first(emu_lib):
    K.check_equal_smallest_eigenvalues_keep_the_first(emu_lib)


def test_all_scores_zero_returns_false_without_a_model(emu_lib):
    K.check_all_scores_zero(emu_lib)


def test_similar_rule_is_strict_at_zero(emu_lib):
    K.check_similar_rule_is_strict(emu_lib)


def test_point_without_parallax_is_counted_not_triangulated(emu_lib):
    K.check_low_parallax_point_is_kept(emu_lib)


def test_non_finite_coordinates(emu_lib):
    K.check_non_finite(emu_lib)


def test_refused_inputs(emu_lib):
    K.check_refused_inputs(emu_lib)


def test_batch_slots_give_the_same_bits(emu_lib):
    K.check_batch_slots(emu_lib)


def test_without_optional_outputs(emu_lib):
    K.check_without_optional_outputs(emu_lib)


def test_repeated_call_gives_the_same_bits(emu_lib):
    K.check_repeat(emu_lib)


def test_three_threads(emu_lib):
    K.check_three_threads(emu_lib)


def test_dropin_cpp_equals_the_c_abi(emu_lib, tmp_path):
    """Initialize on scenes that reconstruct from H, from F, fail either way and are too short; InitializeBatch against the loop of Initialize; the
    draws against the model's restatement of the reference's generator (seeded once a process); Normalize; the scatter to `first`"""
    K.run_cpp(K.build_cpp(tmp_path, emu_lib), emu_lib, tmp_path)


def test_dropin_cpp_under_address_and_undefined_sanitizers(emu_lib, tmp_path):
    """the stand-alone program and the drop-in file built with -fsanitize=address,undefined (the program itself is linked with the sanitizers: nothing
    is preloaded) and run against the emulation library.  The kernels' own file is covered by `make emu_asan` (it is in the Makefile's SRCS)."""
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    env.pop("ASAN_OPTIONS", None)
    K.run_cpp(K.build_cpp(tmp_path, emu_lib, sanitize=True), emu_lib, tmp_path, env=env)
