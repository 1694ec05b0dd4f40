"""orbhip_sim3_optimize (orb_slam2_amd/csrc/orbhip_sim3_opt.hip) under CPU emulation against tests/sim3_opt_model.py: every case of
tests/sim3_opt_cases.py (sizes around the wave, the workgroup and the LDS staging limit, with and without gross outliers, the scale free and fixed, the
named cases) within the recorded spread and, with the model adding in the kernel's own order, bit for bit; bit-for-bit repeatability, batch slots, n == 0 and bad arguments, three threads, the C++ drop-in (also under AddressSanitizer and UBSan as
a stand-alone program).  The checks themselves are in tests/sim3_opt_checks.py, shared with the device run (tests/test_sim3_opt_gpu.py)."""
import pytest

import sim3_opt_cases as Cs
import sim3_opt_checks as K


@pytest.mark.parametrize("name", Cs.ALL_NAMES)
def test_kernel_equals_model(emu_lib, name):
    K.check_case(name, emu_lib)


@pytest.mark.parametrize("name", Cs.ALL_NAMES)
def test_emulated_kernel_equals_the_model_in_the_kernels_order_bit_for_bit(emu_lib, name):
    K.check_case_bits(name, emu_lib)


def test_repeated_call_gives_the_same_bits(emu_lib):
    K.check_repeat(emu_lib)


def test_batch_slots_give_the_same_bits(emu_lib):
    K.check_batch_slots(emu_lib)


def test_no_pairs_touch_nothing_and_bad_arguments_are_refused(emu_lib):
    K.check_empty_and_bad_arguments(emu_lib)


def test_three_threads(emu_lib):
    K.check_three_threads(emu_lib)


def test_dropin_cpp_equals_the_c_abi(emu_lib, tmp_path):
    K.run_cpp(K.build_cpp(tmp_path, emu_lib))


def test_dropin_cpp_under_address_and_undefined_sanitizers(emu_lib, tmp_path):
    """the stand-alone program and the drop-in file built with -fsanitize=address,undefined (the program itself is linked with the sanitizers: nothing
    is preloaded) and run against the emulation library.  The kernels' own file is covered by `make emu_asan` (it is in the Makefile's SRCS)."""
    import os
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    env.pop("ASAN_OPTIONS", None)                                              # defaults: LeakSanitizer checks the drop-in's and the program's allocations too
    K.run_cpp(K.build_cpp(tmp_path, emu_lib, sanitize=True), env=env)
