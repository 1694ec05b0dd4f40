"""orbhip_pnp_iterate (orb_slam2_amd/csrc/orbhip_pnp.hip) under CPU emulation against tests/pnp_model.py: every graded case of tests/pnp_cases.py, where
the emulated kernel must give the model's bits in every hypothesis record, every refine record and the whole answer; the dedicated cases, batch slots,
repeatability, threads, the class's loop and the C++ drop-in (also under AddressSanitizer and UBSan as a
stand-alone program).  The checks themselves are in tests/pnp_checks.py, shared with the device run (tests/test_pnp_gpu.py)."""
import os

import pytest

import pnp_cases as Cs
import pnp_checks as K


@pytest.mark.parametrize("name", Cs.ALL_NAMES)
def test_kernel_equals_model(emu_lib, name):
    K.check_case(name, emu_lib)


def test_generator_conditions():
    K.check_conditions()


def test_cooperative_jacobi_equals_the_serial_template(emu_lib):
    K.check_jacobi_forms(emu_lib)


def test_threshold_is_strict(emu_lib):
    K.check_strict_threshold(emu_lib)


def test_selection_rules(emu_lib):
    K.check_select_rules(emu_lib)


def test_carried_in_mask_is_refined_first(emu_lib):
    K.check_carried_in(emu_lib)


def test_point_behind_the_camera_is_judged_by_the_arithmetic(emu_lib):
    K.check_behind_camera(emu_lib)


def test_coincident_and_collinear_sets(emu_lib):
    K.check_degenerate(emu_lib)


def test_refused_inputs(emu_lib):
    K.check_refused_inputs(emu_lib)


def test_short_problems_touch_nothing(emu_lib):
    K.check_short_untouched(emu_lib)


def test_batch_slots_give_the_same_bits(emu_lib):
    K.check_batch_slots(emu_lib)


@pytest.mark.parametrize("name", Cs.REFINE_NAMES)
def test_refine_equals_model(emu_lib, name):
    K.check_refine_case(name, emu_lib)


def test_sign_rule_reads_the_first_set_bit(emu_lib):
    K.check_sign_first(emu_lib)


@pytest.mark.parametrize("name", K.PASS_SEQUENCES)
def test_selection_across_passes(emu_lib, name):
    K.check_select_passes(name, emu_lib)


def test_fewer_refine_rows_than_refines(emu_lib):
    K.check_ref_cap(emu_lib)


def test_hypothesis_counts_alone(emu_lib):
    K.check_hyp_count_alone(emu_lib)


def test_batch_of_refining_problems(emu_lib):
    K.check_batch_refines(emu_lib)


def test_repeated_call_gives_the_same_bits(emu_lib):
    K.check_repeat(emu_lib)


def test_three_threads(emu_lib):
    K.check_three_threads(emu_lib)


def test_solver_rounds_and_draw_queue(emu_lib):
    K.check_solver_rounds(emu_lib)


def test_dropin_cpp_equals_the_c_abi(emu_lib, tmp_path):
    """the class's rounds over several iterate(5) with the queue and the loop's OR, find, IterateBatch against the loop of iterate, SetRansacParameters"""
    K.run_cpp(K.build_cpp(tmp_path, emu_lib))


def test_dropin_cpp_under_address_and_undefined_sanitizers(emu_lib, tmp_path):
    """the stand-alone program and the drop-in file built with -fsanitize=address,undefined (the program itself is linked with the sanitizers: nothing
    is preloaded) and run against the emulation library.  The kernels' own file is covered by `make emu_asan` (it is in the Makefile's SRCS)."""
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    env.pop("ASAN_OPTIONS", None)
    K.run_cpp(K.build_cpp(tmp_path, emu_lib, sanitize=True), env=env)
