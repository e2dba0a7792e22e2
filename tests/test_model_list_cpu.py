"""The camera-model list (csrc/vg_model_list.hpp) from outside, without a GPU: the model values and intrinsic indices that
tests/test_capi_cpu.py and tests/test_camera_models_cpu.py leave out, and the dispatcher itself in a stand-alone program."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNKNOWN = (-1, 3, 6)
FOCAL = (1.0, 1e5)       # fu, fv, u0, v0 of every model
DISTORTION = (-10.0, 10.0)
# vg_intrinsic_bounds as it stood before the model list, written out; the pairs the two files above assert already are left out
BOUNDS = {(0, 3): FOCAL, (0, 4): FOCAL, (0, 5): FOCAL,
          (1, 1): FOCAL, (1, 2): FOCAL, (1, 3): FOCAL,
          (2, 1): DISTORTION, (2, 2): DISTORTION, (2, 4): DISTORTION, (2, 7): FOCAL, (2, 8): FOCAL, (2, 9): FOCAL}


@pytest.fixture(scope="module")
def L():
    from visgeom_amd import capi

    return capi.load()


def test_counts_of_the_values_next_to_the_list(L):
    assert [L.vg_num_intrinsics(m) for m in (-1, 6, 7, -2 ** 31, 2 ** 31 - 1)] == [-1] * 5


def test_bounds_of_the_remaining_indices(L):
    from visgeom_amd import capi

    lo, hi = ctypes.c_double(), ctypes.c_double()
    for (m, i), want in BOUNDS.items():
        assert L.vg_intrinsic_bounds(m, i, ctypes.byref(lo), ctypes.byref(hi)) == 0, (m, i)
        assert (lo.value, hi.value) == want, (m, i)
    for m, K in ((0, 6), (2, 10), (4, 8)):   # one past the end, and in front of the start
        for i in (K, -1):
            assert L.vg_intrinsic_bounds(m, i, ctypes.byref(lo), ctypes.byref(hi)) == capi.ERR_INVALID_ARGUMENT, (m, i)


@pytest.mark.parametrize("m", UNKNOWN)
def test_bounds_refuse_an_unknown_model_at_every_index(L, m):
    from visgeom_amd import capi

    for i in range(10):
        if (m, i) == (3, 0):   # tests/test_camera_models_cpu.py
            continue
        lo, hi = ctypes.c_double(-7.0), ctypes.c_double(-7.0)
        assert L.vg_intrinsic_bounds(m, i, ctypes.byref(lo), ctypes.byref(hi)) == capi.ERR_INVALID_ARGUMENT, (m, i)
        assert (lo.value, hi.value) == (-7.0, -7.0)


DISPATCH_PROGRAM = r"""
#include "vg_model_list.hpp"
#include <cstdio>
template <int... MS>
int check(vg::ModelList<MS...> list, const char *name)
{
    int bad = 0;
    for (int model = -3; model <= 8; model++) {
        int calls = 0, got = -100;
        const bool hit = vg::dispatch_model(model, list, [&](auto m) { calls++; got = decltype(m)::value; });
        const bool listed = (... || (model == MS));
        if (hit != listed || calls != (listed ? 1 : 0) || (listed && got != model) || vg::model_in(model, list) != listed) {
            std::printf("%s: model %d: returned %d after %d calls with %d\n", name, model, (int)hit, calls, got);
            bad++;
        }
    }
    return bad;
}
static_assert(vg::num_intrinsics(0) == 6 && vg::num_intrinsics(1) == 5 && vg::num_intrinsics(2) == 10 && vg::num_intrinsics(4) == 8 &&
              vg::num_intrinsics(5) == 6 && vg::num_intrinsics(3) == -1 && vg::num_intrinsics(-1) == -1 && vg::num_intrinsics(6) == -1, "");
static_assert(vg::CameraTraits<vg::kEUCM>::kFocal == 2 && vg::CameraTraits<vg::kUCM>::kFocal == 1 && vg::CameraTraits<vg::kMEI>::kFocal == 6 &&
              vg::CameraTraits<vg::kKB>::kFocal == 4 && vg::CameraTraits<vg::kDS>::kFocal == 2, "");
int main()
{
    const int bad = check(vg::AllModels{}, "all") + check(vg::ReferenceModels{}, "reference") + check(vg::AddedModels{}, "added");
    std::printf("%d\n", bad);
    return bad ? 1 : 0;
}
"""


def test_dispatcher_in_a_stand_alone_program(tmp_path):
    """every listed value: one call with that value, true; every other value: no call, false; for each of the three lists"""
    src, exe = tmp_path / "dispatch.cpp", tmp_path / "dispatch"
    src.write_text(DISPATCH_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "visgeom_amd", "csrc"),
                           str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).strip() == "0"
