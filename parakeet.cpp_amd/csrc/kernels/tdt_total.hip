// parakeet.cpp_amd/csrc/kernels/tdt_total.hip -- the forward-algorithm total of a GIVEN token string under the TDT head.
//
// The specification is tests/tdt_total_ref.py: the lattice and the arcs of the TDT forced alignment (kernels/tdt_align.hip, tests/tdt_align_ref.py),
// walked sum-product in pull form: alpha[0][0] = 0, every other cell a left fold with lae (m + dlogf(1 + dexpf(n - m)), m where n == -inf: the one
// kernels/ctc_align.hip uses) from -inf over the candidates blank 0 .. D-1 then label 0 .. D-1, each alpha[src] + (x + dl) as two fp32 adds; a blank
// of duration 0 and a blank of duration 1 are two arcs to t + 1 and both are summed.  END is the same fold over the source frames in ascending
// order, blank before label, then by i.  The value is compared bit for bit.
//
//   tdt_total_kernel<NT>      one workgroup of NT threads per hypothesis: tdt_lattice_walk (tdt_lattice_dev.hpp, which describes it) with the log-sum
//       fold -- the walk tdt_align_kernel has written out with its max-plus fold.  Nothing is written per cell: no back-pointers, no back-trace.
//       total[b] = END, ok[b] = END > -inf.
//
// Limits (host side: tdt_total.cpp refuses with PK_ERR_UNSUPPORTED before anything is allocated): those of the alignment -- durations in
//   [0, kTdtAlignMaxDur = 8], 1 <= D <= 8, U_b <= kTdtAlignMaxTokens = 1535 (ring of (8 + 2) x 1536 x 4 = 61440 bytes of LDS), scratch of a call or of
//   a group of hypotheses <= 1 GiB (formula: tdt_total.hpp, the alignment's without the back-pointer bytes).
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   tdt_total_kernel< 64>       41 VGPR 106 SGPR  LDS 64 B + the ring  scratch 0 B; 0 VGPR spills, 53 SGPRs spilled to VGPR lanes
//   tdt_total_kernel<256>       41 VGPR 106 SGPR  LDS 64 B + the ring  scratch 0 B; 0 VGPR spills, 53 SGPRs spilled to VGPR lanes
//   (as in tdt_align_kernel the durations and blank steps are wave-uniform and live in SGPRs; nothing goes to private memory)
//   (the ring: (dur_max + 2) (u_max + 1) 4 bytes of dynamic LDS, 3 KB for 90 tokens and durations up to 4, 61440 bytes at the limits)
#include "tdt_lattice_dev.hpp"

namespace pk {

template <int NT>
__global__ __launch_bounds__(NT) void tdt_total_kernel(TdtTotalArgs a) {
    extern __shared__ float ring[];                                 // [dur_max + 2][u_max + 1]
    __shared__ float tail[2][kTdtAlignMaxDur];                      // alpha[T - 8 + j][U - 1 + c]: what END pulls from
    const int b = blockIdx.x;
    const TdtLogSum end = tdt_lattice_walk<NT, TdtLogSum>(a.lt, b, a.u_max, a.dur_max, ring, tail);
    if (threadIdx.x == 0) {
        a.total[b] = end.v;
        a.ok[b] = end.v > -__builtin_huge_valf() ? 1 : 0;
    }
}

void launch_tdt_total(const TdtTotalArgs &a, hipStream_t s) {
    const size_t lds = tdt_walk_launch_checks("launch_tdt_total", a.lt, a.u_max, a.dur_max);
    if (a.lt.B <= 0) return;
    if (a.u_max + 1 <= kTdtAlignThreads[0]) hipLaunchKernelGGL(tdt_total_kernel<64>, dim3(a.lt.B), dim3(64), lds, s, a);
    else hipLaunchKernelGGL(tdt_total_kernel<256>, dim3(a.lt.B), dim3(256), lds, s, a);
}

}  // namespace pk
