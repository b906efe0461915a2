// Device-code-only translation unit for tests/test_isa_audit_q4.py: 4-bit GPTQ instantiations of the streaming decode kernel (WT = 3), each next
// to the 16-bit instantiation (WT = 1) of the same form.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S q4_isa_probe.hip
#include "../../bitdelta_amd/csrc/bd_gemv_stream.h"
// each pair at its SHIPPED prefetch depth (launch_gemv_stream_chunk): with one or two tenants the 4-bit form runs four times the stages of its
// 16-bit twin where the activation rows are resident (a stage is then 3 loads), twice where every stage loads its own activation fragments
//               DT, NM,  NS16, NSQ,  XL, EPI, FG        (HASW, 4 waves, natural order, nt weight loads, packed layout)
#define BD_PAIR(DT, NM, NS16, NSQ, XL, EPI, FG)                                                                              \
    template __global__ void bd::gemv_stream_kernel<DT, NM, true, NS16, 4, 1, 2, 1, XL, EPI, 1, FG>(const bd::StreamParams);  \
    template __global__ void bd::gemv_stream_kernel<DT, NM, true, NSQ, 4, 1, 2, 1, XL, EPI, 3, FG>(const bd::StreamParams);
BD_PAIR(bd::DT_F16, 6, 4, 4, 0, 0, 0)          // down projection of a 6-tenant step: per-stage activation loads
BD_PAIR(bd::DT_BF16, 1, 3, 6, 0, 0, 0)         // one tenant, plain
BD_PAIR(bd::DT_BF16, 6, 2, 2, 1, 1, 0)         // RMSNorm prologue + SwiGLU epilogue
BD_PAIR(bd::DT_F16, 6, 2, 2, 2, 0, 0)          // o projection: resident rows
BD_PAIR(bd::DT_BF16, 8, 2, 2, 3, 1, 0)         // hand-off consumer with the SwiGLU epilogue, 8 tenants
BD_PAIR(bd::DT_F16, 6, 2, 2, 3, 0, 1)          // fine grid: q|k|v of a 6-tenant step (hand-off consumer)
BD_PAIR(bd::DT_BF16, 6, 2, 2, 2, 1, 1)         // fine grid: resident rows with the SwiGLU epilogue
BD_PAIR(bd::DT_F16, 1, 2, 8, 3, 1, 0)          // one tenant: gate|up, hand-off consumer with the SwiGLU epilogue
BD_PAIR(bd::DT_BF16, 2, 2, 8, 3, 0, 1)         // two tenants, fine grid
BD_PAIR(bd::DT_BF16, 1, 2, 8, 1, 0, 0)         // one tenant: RMSNorm prologue
