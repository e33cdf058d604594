// dtof_shade_mesh.hip -- instantiations of k_shade (dtof_shade.h): diffuse scenes with triangle meshes / analytic shapes (MESH = true, SPEC = 0).
#include "dtof_shade.h"

namespace dtof {

void launch_shade_mesh(bool area, bool k4, const ShadeLaunch &L) {
    if (area) { if (k4) launch_shade_variant<true, kMaxOffsets, true, 0>(L); else launch_shade_variant<true, 1, true, 0>(L); }
    else      { if (k4) launch_shade_variant<false, kMaxOffsets, true, 0>(L); else launch_shade_variant<false, 1, true, 0>(L); }
}

// dtof_emitter_eval, levels 2 (no area emitters) and 3 (area emitters) (k_emitter_eval in dtof_shade.h)
void launch_emitter_eval_mesh(const uint8_t *scene, int level, int mode, uint32_t index, float pmf, const float *in, float *out, uint32_t n, hipStream_t s) {
    if (level == 3) launch_emitter_eval_level<true, true, 0>(scene, mode, index, pmf, in, out, n, s); else launch_emitter_eval_level<false, true, 0>(scene, mode, index, pmf, in, out, n, s);
}

}  // namespace dtof
