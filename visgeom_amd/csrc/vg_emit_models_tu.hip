// vg_emit_models_tu.hip -- translation unit of libvisgeom_amd.so: the emit launches of the camera models that are not in the
// reference, Kannala-Brandt and double sphere.  The same kernel template and launch rules as the
// reference's three models (vg_kernels.hpp, vg_emit_launch.hpp), instantiated here so that vg_emit_tu.hip builds what it built
// before and the two units compile side by side.  Built with hipcc for gfx950 only.
#define VG_TU_EMIT_MODELS  // of vg_emit_launch.hpp only the launch templates: the reference models' dispatch and the merged launch stay in vg_emit_tu.hip
#include "vg_emit_launch.hpp"

int vgi::launch_emit_added_model(hipStream_t stream, int model, const vg::EmitArgs &a, bool want_jac, bool inline_chain)
{
    int rc = VG_OK;
    const bool here = vg::dispatch_model(model, vg::AddedModels{}, [&](auto m) { rc = launch_emit<decltype(m)::value>(stream, a, want_jac, inline_chain); });
    return here ? rc : fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
}
