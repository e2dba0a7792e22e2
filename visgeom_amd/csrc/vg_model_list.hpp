// vg_model_list.hpp -- the camera models as ONE list: their ids, their intrinsic counts, and the step from a run-time `int model`
// to a template argument that every host launch site takes (dispatch_model).  Plain C++17: no HIP in here.
//
// Adding a camera model: the enum, CameraTraits and the lists below; eval_corner / eval_corner_fast
// (vg_camera.hpp); the structural zero pattern intr_nonzero (vg_gram_valu.hpp); vg_intrinsic_bounds (vg_problem_tu.hip);
// reconstruct_point and the JSON type names (vg_calibration.hpp); VG_MODEL_* (include/visgeom_amd.h), capi.py and the name
// parse of rectify_main.cpp.  Moving a model from AddedModels to ReferenceModels also takes a case in the two device-side
// switches (vg_emit_multi_kernel, the merged Gram kernel).
#pragma once

#include <type_traits>

namespace vg {

// Kannala-Brandt and double sphere are not in the reference; value 3 stays unassigned and refused
enum Model : int { kEUCM = 0, kUCM = 1, kMEI = 2, kKB = 4, kDS = 5 };

template <int N>
struct Intrinsics {
    static constexpr int K = N;
    static constexpr int kFocal = N - 4;  // every model ends in fu, fv, u0, v0: intrinsics[kFocal .. kFocal + 3]
};
template <int MODEL>
struct CameraTraits;
template <> struct CameraTraits<kEUCM> : Intrinsics<6> {};
template <> struct CameraTraits<kUCM> : Intrinsics<5> {};
template <> struct CameraTraits<kMEI> : Intrinsics<10> {};
template <> struct CameraTraits<kKB> : Intrinsics<8> {};
template <> struct CameraTraits<kDS> : Intrinsics<6> {};

template <int... MS>
struct ModelList {};
using ReferenceModels = ModelList<kEUCM, kUCM, kMEI>;  // the merged launches and the localization costs are built for these
using AddedModels = ModelList<kKB, kDS>;               // their emit kernels live in vg_emit_models_tu.hip
using AllModels = ModelList<kEUCM, kUCM, kMEI, kKB, kDS>;

// f(std::integral_constant<int, M>{}) for the one M of the list that equals `model`; false, and no call, when none does.
// A LEFT fold: the compiler then instantiates what f launches in the order of the list, which is the order of the kernels in the
// unit's code object (a right fold lays them out last model first).
template <int... MS, class F>
constexpr bool dispatch_model(int model, ModelList<MS...>, F &&f)
{
    return (... || (model == MS && (f(std::integral_constant<int, MS>{}), true)));
}

template <int... MS>
constexpr bool model_in(int model, ModelList<MS...>)
{
    return (... || (model == MS));
}

// -1 for a model that is not in the list (at most one term of the sum is not zero)
template <int... MS>
constexpr int num_intrinsics(int model, ModelList<MS...>)
{
    return ((model == MS ? CameraTraits<MS>::K + 1 : 0) + ...) - 1;
}
constexpr int num_intrinsics(int model) { return num_intrinsics(model, AllModels{}); }

}  // namespace vg
