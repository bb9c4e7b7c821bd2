// Device pieces shared by the flash-attention kernel files (attention.hip,
// attention256.hip): the strided [B, S, H, D] view, the accumulator row map of
// the 32 x 32 MFMA, the 16-byte row store of a C^T tile and the XCD-local
// order of a non-causal grid.
#pragma once
#include "mfma.h"

namespace ffk {

// A [B, S, H, D] tensor: element strides for b / s / h, d contiguous.
template <class T>
struct TensorViewT {
  T* p;
  int64_t sb, ss, sh;
  __device__ __forceinline__ T* row(int b, int s, int h) const { return p + b * sb + static_cast<int64_t>(s) * ss + h * sh; }
};
using TensorView = TensorViewT<const bf16>;
using OutView = TensorViewT<bf16>;

constexpr float kLog2e = 1.4426950408889634f;

// Row of register r of a 32 x 32 MFMA accumulator, before the lane half's
// + 4 h: registers 4g .. 4g+3 hold rows 8g .. 8g+3.
__device__ constexpr int acc_row(int r) { return (r & 3) + 8 * (r >> 2); }

// Store a wave's 32-row C^T tile (lane & 31 -> row, registers -> d) as rows
// of bf16, 16 bytes per store.  A lane holds 4 consecutive d of each 8-group
// (lane half h: d = 8 g + 4 h + e); v_permlane32_swap trades group 2p+1 of
// the lower half for group 2p of the upper half, so after the swap every
// lane holds 8 consecutive d (lower half: d 16p..16p+7 = its own group 2p
// and its partner's; upper half: 16p+8..16p+15) -- half the store
// instructions of the 8-byte form (the epilogue tail is store-issue bound,
// guide T21).  Every lane runs the swaps; `ok` guards only the stores.
template <int DT>
__device__ __forceinline__ void store_rows16(bf16* row, const f32x16 (&acc)[DT], float mul, int h, bool ok) {
  auto pk = [](float a, float b) -> unsigned {
    return static_cast<unsigned>(f2u(a)) | (static_cast<unsigned>(f2u(b)) << 16);
  };
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      const int ga = 2 * gp, gb = 2 * gp + 1;
      const unsigned xa0 = pk(acc[dt][4 * ga + 0] * mul, acc[dt][4 * ga + 1] * mul);
      const unsigned xa1 = pk(acc[dt][4 * ga + 2] * mul, acc[dt][4 * ga + 3] * mul);
      const unsigned yb0 = pk(acc[dt][4 * gb + 0] * mul, acc[dt][4 * gb + 1] * mul);
      const unsigned yb1 = pk(acc[dt][4 * gb + 2] * mul, acc[dt][4 * gb + 3] * mul);
      const auto s0 = __builtin_amdgcn_permlane32_swap(xa0, yb0, false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(xa1, yb1, false, false);
      if (ok) {
        u32x4t v = {static_cast<unsigned>(s0[0]), static_cast<unsigned>(s1[0]), static_cast<unsigned>(s0[1]),
                    static_cast<unsigned>(s1[1])};
        *reinterpret_cast<u32x4t*>(row + dt * 32 + 16 * gp + 8 * h) = v;
      }
    }
}

// (head, block) of a non-causal workgroup, grid (blocks, B*H).  Dispatch puts
// linear id L = x + y * gridDim.x on XCD L % 8, so without a remap the
// blocks of one head (4 query blocks at S = 512) run on four XCDs and every
// XCD's L2 fetches that head's K / V.  The bijective remap (mfma.h) gives
// each XCD a contiguous range of linear ids, i.e. whole heads: a head's K / V
// come from HBM once and its other blocks hit in the XCD's L2.
__device__ __forceinline__ void attn_head_block(int& bh, int& blk) {
  const int W = gridDim.x * gridDim.y;
  const int r = xcd_remap(blockIdx.x + blockIdx.y * gridDim.x, W);
  bh = r / gridDim.x;
  blk = r % gridDim.x;
}

}  // namespace ffk
