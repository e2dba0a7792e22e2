// vg_emit_models_tu.hip -- translation unit of libvisgeom_amd.so: the emit launches of the camera models that are not in the
// reference, Kannala-Brandt and double sphere.  The same kernel template and launch rules as the
// reference's three models (vg_kernels.hpp, vg_emit_launch.hpp), instantiated here so that vg_emit_tu.hip builds what it built
// before and the two units compile side by side.  Built with hipcc for gfx950 only.
#define VG_TU_EMIT_MODELS  // of vg_emit_launch.hpp only the launch templates: the model switch and the merged launch stay in vg_emit_tu.hip
#include "vg_emit_launch.hpp"

int vgi::launch_emit_added_model(hipStream_t stream, int model, const vg::EmitArgs &a, bool want_jac, bool inline_chain)
{
    switch (model) {
    case VG_MODEL_KB: return launch_emit<vg::kKB>(stream, a, want_jac, inline_chain);
    case VG_MODEL_DS: return launch_emit<vg::kDS>(stream, a, want_jac, inline_chain);
    default: return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
    }
}
