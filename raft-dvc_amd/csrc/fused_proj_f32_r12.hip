// fused_proj_f32_r12.hip -- the r = 1 and r = 2 instances of k_fused_proj_f32 (fused_proj_f32.hip), compiled without
// SLP vectorisation: with it hipcc forms one packed-FP32 add per instance whose low lane reads the high half of a
// pair, the op that returned wrong low-lane values while another wave ran MFMAs (round 2; tools/isa_check.py).  The
// r = 3 and r = 4 instances compile clean with SLP, as the other radii of k_fused_proj do (fused_proj_r1.hip).
#define DVC_FPROJ_F32_R12_TU 1
#include "fused_proj_f32.hip"

namespace dvc {
#define DVC_FPROJ_F32_R12_INST(R, KS)                                                                        \
    template __global__ void k_fused_proj_f32<R, KS>(const float *, const float *, LookupArgs,               \
                                                     const unsigned long long *, int, int, long long, float, float *);
DVC_FPROJ_F32_R12_INST(1, 1) DVC_FPROJ_F32_R12_INST(1, 2) DVC_FPROJ_F32_R12_INST(1, 4)
DVC_FPROJ_F32_R12_INST(2, 1) DVC_FPROJ_F32_R12_INST(2, 2) DVC_FPROJ_F32_R12_INST(2, 4)
}  // namespace dvc
