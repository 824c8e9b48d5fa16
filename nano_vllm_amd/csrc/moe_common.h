// What the two expert paths of the Qwen3-MoE block (moe.hip: bf16 weights, moe_mxfp4.hip: MXFP4 weights) share: the
// limits, the workspace layout that nvl_moe_plan fills, the shape check and the combine launch.
#pragma once
#include "common.h"

namespace {

constexpr int kRowBlock = 128;           // rows per row block (8 MFMA row tiles)
constexpr int kMaxE = 256;
constexpr int kMaxTopK = 8;

struct MoeLayout {
  size_t offsets, sorted, pos, blocks, h, y, index_end, total;
  int64_t pairs;
  int64_t nb_max;
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Workspace of a call with m tokens: the index section depends on (m, E, top_k) only (nvl_moe_plan knows nothing else).
inline MoeLayout moe_layout(int64_t m, int hidden, int inter, int E, int top_k) {
  MoeLayout l;
  l.pairs = m * top_k;
  l.nb_max = l.pairs / kRowBlock + (l.pairs < E ? l.pairs : E);
  size_t o = 0;
  l.offsets = o; o = align256(o + (size_t)(E + 1) * 4);
  l.sorted = o;  o = align256(o + (size_t)l.pairs * 4);
  l.pos = o;     o = align256(o + (size_t)l.pairs * 4);
  l.blocks = o;  o = align256(o + (size_t)l.nb_max * 16);
  l.index_end = o;
  l.h = o;       o = align256(o + (size_t)l.pairs * inter * 2);
  l.y = o;       o = align256(o + (size_t)l.pairs * hidden * 4);
  l.total = o;
  return l;
}

__device__ __forceinline__ float silu_f32(float g) { return g / (1.f + __expf(-g)); }

inline bool moe_shape_ok(int64_t m, int E, int top_k, const char* who) {
  if (!(m >= 0 && m <= (1 << 20) && E >= 1 && E <= kMaxE && top_k >= 1 && top_k <= kMaxTopK && top_k <= E)) {
    nvl_set_error("%s: m=%lld E=%d top_k=%d: need 0 <= m <= 2^20, 1 <= E <= 256, 1 <= top_k <= 8, top_k <= E", who,
                  (long long)m, E, top_k);
    return false;
  }
  return true;
}

}  // namespace

// out[t] = bf16(sum_j topk_w[t, j] * y[pos[t, j]]), slots in order, fp32 (moe_combine_kernel, moe.hip).
void moe_launch_combine(const float* y, const int* pos, const float* topk_w, void* out, int64_t m, int hidden, int top_k,
                        int pairs, hipStream_t stream);
