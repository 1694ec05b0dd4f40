"""orbhip_pose_optimization (orb_slam2_amd/csrc/orbhip_pose_opt.hip) under CPU emulation against tests/pose_opt_model.py: every case of
tests/pose_opt_cases.py (sizes around the wave, the workgroup and the LDS staging limit; monocular, stereo and mixed edges; with and without gross
outliers; initial rotations past 120 degrees; every edge an outlier, zero residuals, points behind the camera, a float-product pose), bit-for-bit repeatability, batch slots, the frame form, the short cases, the C++ drop-in (also under AddressSanitizer and UBSan as a stand-alone
program).  The checks themselves are in tests/pose_opt_checks.py, shared with the device run (tests/test_pose_opt_gpu.py)."""
import numpy as np
import pytest

import orb_slam2_amd
import pose_opt_cases as Cs
import pose_opt_checks as K
import pose_opt_model as M


@pytest.mark.parametrize("name", Cs.ALL_NAMES)
def test_kernel_equals_model(emu_lib, name):
    K.check_case(name, emu_lib)


def test_repeated_call_gives_the_same_bits(emu_lib):
    K.check_repeat(emu_lib)


def test_batch_slots_give_the_same_bits(emu_lib):
    K.check_batch_slots(emu_lib)


def test_batch_of_size_and_degenerate_cases(emu_lib):
    K.check_batch_edges(emu_lib)


def test_frame_form_equals_host_array_form(emu_lib):
    K.check_frame_form(emu_lib)


def test_fewer_than_three_observations_touch_nothing(emu_lib):
    K.check_short_untouched(emu_lib)


def test_three_threads(emu_lib):
    K.check_three_threads(emu_lib)


def test_point_at_the_camera_centre_returns_and_equals_the_model(emu_lib):
    """a point exactly at the initial camera centre: z = 0, a non-finite chi2 from the first evaluation on.  Every loop of the kernel is bounded by a
    constant, so the call returns; and it does what the model does with the same non-finite numbers."""
    from test_pose_opt_model import camera_centre_problem
    cam, T0, obs = camera_centre_problem()
    Tm, fm, nm, tr = M.pose_optimization(cam, T0, obs, want_trace=True)
    # This is the one kernel test that tells a classification at the rejected trial's pose (PoState::last) from one at the estimate: every trial pose is
    # NaN here, so the stale rule flags nothing, and fresh errors at the estimate would flag many.  No grid case can tell the two: their edges lie more
    # than 1e-6 from the thresholds and a tenth rejected step moves chi2 by far less.
    init = M.to_se3quat(T0)
    fresh, _ = M.classify(M.Problem(cam, obs), np.zeros(len(obs), bool), init, init, fresh=True)
    assert tr["stale_matters"] and fm.sum() == 0 and fresh.sum() >= 20
    Td, fd, nd = orb_slam2_amd.pose_optimization(cam, T0, obs, library=emu_lib)
    assert np.array_equal(fd, fm) and nd == nm
    assert np.array_equal(np.isfinite(Td), np.isfinite(Tm)) and np.array_equal(Td[np.isfinite(Td)], Tm[np.isfinite(Tm)])


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
