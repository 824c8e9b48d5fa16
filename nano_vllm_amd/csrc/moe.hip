// Sparse mixture-of-experts feed-forward block of Qwen3-MoE (Qwen3-30B-A3B: 128 experts, 8 per token, hidden 2048,
// expert width 768) for gfx950: router, expert sort and grouped expert GEMMs. A dense decode GEMM cannot express "a
// different weight matrix per row", and a host loop over the experts cannot live in a captured graph because the row
// counts per expert are device data. Here every grid is a function of the host-known shapes only:
//
//   nvl_moe_route    one WAVE per token. The token's x row sits in registers as fp32 (hidden / 64 values per lane); the
//                    router matrix ([E, hidden], 512 KiB for 30B-A3B: L2-resident) is walked 16 experts at a time with
//                    a transposing wave reduction, logit e parked in lane e % 64, register e / 64. Softmax over all E in
//                    fp32, then top_k rounds of a wave arg-max (larger p first, LOWER index on ties) — no sort.
//   nvl_moe_plan     stable counting sort of the m * top_k (token, slot) pairs by expert, no atomics: workgroup e walks
//                    the pair list twice — once counting the pairs of experts < e (its offset) and of e, once compacting
//                    its own pairs with wave ballots in pair order. A one-workgroup kernel then cuts every expert's run
//                    of sorted rows into ROW BLOCKS of <= 128 rows and pads the list to its static bound
//                    floor(P / 128) + min(E, P); a padded entry has 0 rows.
//   nvl_moe_experts  (a) gate|up GEMM + SiLU * mul, (b) down GEMM, (c) combine: three launches.
//                    GEMM work item = (row block, column group), 4 waves. The block's <= 128 rows (<= 8 MFMA row tiles)
//                    are staged per 128-wide k step in LDS — 256 B per row, 16-byte chunks XOR-swizzled with the row so
//                    that the 16 rows a B-fragment read touches cover all 64 banks; in (a) the rows are GATHERED by token
//                    id, in (b) they are contiguous in sorted order — two stages, the global loads of step s + 1 are in
//                    flight under the MFMAs of step s, one barrier per step. Each wave owns two 16-column weight tiles
//                    ((a): a gate tile and ITS up tile, paired in registers for the epilogue) and streams their A
//                    fragments global -> VGPR one step ahead, consuming them against ALL row tiles of the block: an
//                    expert's weights are read once per 128 pairs, not once per 16-row tile.
//                    v_mfma_f32_16x16x32_bf16, A = W fragment, B = x fragment: lane (l15, lq) holds
//                    out[row 16 mt + l15][col tile + 4 lq .. + 3] (as gemm_wide.hip).
//                    (c) out[t] = bf16(sum over the token's slots IN SLOT ORDER of w[t, j] * y[pos(t, j)]) in fp32: no
//                    atomics anywhere, every sum has one fixed order => bit-identical from run to run, and a row's
//                    result does not depend on which block it landed in.
//   Surplus workgroups (padded row blocks) leave as a whole before the first barrier.
// Rounding points are nvl_linear_decode's: gate and up are rounded to bf16 before the activation, h is bf16, the down
// projection stays fp32 until the combine rounds once.
// (nvl_moe_experts_mxfp4, the same three launches over 4-bit expert weights, is moe_mxfp4.hip; moe_common.h holds what
// the two share.)
#include "moe_common.h"

namespace {

// ---- router -------------------------------------------------------------------------------------------------------
// One wave (= one workgroup) per token. HC = 16-byte chunks of the x row per lane (hidden <= HC * 512), held as fp32.
// Experts are taken 16 at a time: every lane accumulates its part of the 16 dot products (16 x HC coalesced 1-KiB wave
// loads in flight), then a TRANSPOSING reduction — four halving exchanges (lane ^ 32, 16, 8, 4: each lane keeps the half
// of its values its lane bit selects and adds the partner's) and two plain ones (lane ^ 2, 1) — leaves the logit of
// expert e0 + j in lanes 4 j .. 4 j + 3: 18 cross-lane moves per 16 experts instead of 96.
template <int HC>
__global__ __launch_bounds__(64) void moe_route_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ rw,
                                                       int* __restrict__ ids, float* __restrict__ wts, int64_t m,
                                                       int hidden, int E, int top_k, int norm) {
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  const int nchunks = hidden >> 3;
  float xr[HC][8];
#pragma unroll
  for (int i = 0; i < HC; ++i) {
    // (a chunk past the row: chunk c % 16 is read instead — always there, hidden % 128 == 0 — and x counts as zero, so
    //  every load below is unconditional: a load under a lane-dependent branch is waited for inside that branch, and
    //  the 16 x HC loads of a group would become one latency chain)
    const int c = i * 64 + lane;
    u32x4_t v = *reinterpret_cast<const u32x4_t*>(x + t * hidden + (c < nchunks ? c : c & 15) * 8);
    if (c >= nchunks) v = u32x4_t{0u, 0u, 0u, 0u};
    unpack8(v, xr[i]);
  }
  float lg[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int e0 = 0; e0 < E; e0 += 16) {
    float a[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int e = e0 + j < E ? e0 + j : E - 1;                // (a group's rows past E: a valid row, never parked)
      const bf16_t* row = rw + (int64_t)e * hidden;
      a[j] = 0.f;
#pragma unroll
      for (int i = 0; i < HC; ++i) {
        const int c = i * 64 + lane;
        float wv[8];
        unpack8(*reinterpret_cast<const u32x4_t*>(row + (c < nchunks ? c : c & 15) * 8), wv);
#pragma unroll
        for (int q = 0; q < 8; ++q) a[j] = fmaf(xr[i][q], wv[q], a[j]);
      }
    }
#pragma unroll
    for (int st = 0; st < 4; ++st) {                            // 16 -> 8 -> 4 -> 2 -> 1 values per lane
      const int n = 8 >> st, mask = 32 >> st;
      const bool upper = (lane & mask) != 0;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i < n) {
          const float keep = upper ? a[i + n] : a[i];
          const float send = upper ? a[i] : a[i + n];
          a[i] = keep + __shfl_xor(send, mask, 64);
        }
    }
    a[0] += __shfl_xor(a[0], 2, 64);
    a[0] += __shfl_xor(a[0], 1, 64);
    const float mine = __shfl(a[0], (lane & 15) << 2, 64);      // expert e0 + (lane & 15) sits in lanes 4 (lane & 15) ...
    const bool park = (lane >> 4) == ((e0 >> 4) & 3) && e0 + (lane & 15) < E;   // ... and is parked in lane e % 64
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (park && s == (e0 >> 6)) lg[s] = mine;
  }
  float mx = fmaxf(fmaxf(lg[0], lg[1]), fmaxf(lg[2], lg[3]));
  mx = wave_allreduce_max(mx);
  float p[4], psum = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    p[s] = s * 64 + lane < E ? expf(lg[s] - mx) : -1.f;           // -1: not an expert / already taken
    psum += p[s] > 0.f ? p[s] : 0.f;
  }
  psum = wave_allreduce_sum(psum);
  const float inv = 1.f / psum;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (p[s] >= 0.f) p[s] *= inv;
  float sel_p = 0.f, ssum = 0.f;
  int sel_id = 0;
  for (int j = 0; j < top_k; ++j) {
    float bv = -2.f;
    int bi = 0x7fffffff;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (p[s] > bv) { bv = p[s]; bi = s * 64 + lane; }           // strict: the lower slot wins a tie
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (bi >= E || bi < 0) { bi = j; bv = 0.f; }                  // (a NaN row: still E-bounded ids)
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (bi == s * 64 + lane) p[s] = -1.f;
    if (lane == j) { sel_id = bi; sel_p = bv; }
    ssum += bv;
  }
  if (lane < top_k) {
    ids[t * top_k + lane] = sel_id;
    wts[t * top_k + lane] = norm ? sel_p / ssum : sel_p;
  }
}

// ---- plan ---------------------------------------------------------------------------------------------------------
// Workgroup e: offsets[e] = pairs of experts < e; its own pairs, in pair order, to sorted[offsets[e] ...]; pos = inverse.
__global__ __launch_bounds__(256) void moe_sort_kernel(const int* __restrict__ ids, int P, int E, int* __restrict__ offsets,
                                                       int* __restrict__ sorted, int* __restrict__ pos) {
  __shared__ int s_lt[4], s_eq[4];
  const int e = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int per = (((P + 3) >> 2) + 63) & ~63;                    // pairs per wave: four contiguous quarters
  const int lo = wave * per, hi = lo + per < P ? lo + per : P;
  int lt = 0, eq = 0;
  for (int base = lo; base < hi; base += 64) {
    const int i = base + lane;
    const int id = i < hi ? ids[i] : -1;
    lt += __popcll(__builtin_amdgcn_ballot_w64(id >= 0 && id < e));
    eq += __popcll(__builtin_amdgcn_ballot_w64(id == e));
  }
  if (lane == 0) { s_lt[wave] = lt; s_eq[wave] = eq; }
  __syncthreads();
  const int off = s_lt[0] + s_lt[1] + s_lt[2] + s_lt[3];
  int run = off;
  for (int w = 0; w < wave; ++w) run += s_eq[w];
  if (threadIdx.x == 0) {
    offsets[e] = off;
    if (e == E - 1) offsets[E] = off + s_eq[0] + s_eq[1] + s_eq[2] + s_eq[3];
  }
  for (int base = lo; base < hi; base += 64) {
    const int i = base + lane;
    const int id = i < hi ? ids[i] : -1;
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(id == e);
    if (id == e) {
      const int r = run + __popcll(mask & ((1ull << lane) - 1ull));
      if (r < P) { sorted[r] = i; pos[i] = r; }
    }
    if (e == 0 && i < hi && (id < 0 || id >= E)) pos[i] = -1;     // an id outside [0, E): the pair contributes nothing
    run += __popcll(mask);
  }
}

// One workgroup: row blocks (expert, first sorted row, rows <= 128, 0) of every expert, padded with empty blocks.
__global__ __launch_bounds__(256) void moe_blocks_kernel(const int* __restrict__ offsets, int E, int* __restrict__ blocks,
                                                         int nb_max) {
  __shared__ int scan[256];
  const int e = threadIdx.x;
  int first = 0, cnt = 0;
  if (e < E) { first = offsets[e]; cnt = offsets[e + 1] - first; }
  const int nb = (cnt + kRowBlock - 1) / kRowBlock;
  scan[e] = nb;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int v = e >= d ? scan[e - d] : 0;
    __syncthreads();
    scan[e] += v;
    __syncthreads();
  }
  const int start = scan[e] - nb, total = scan[255];
  for (int b = 0; b < nb; ++b) {
    const int i = start + b;
    if (i < nb_max) {
      const int rows = cnt - b * kRowBlock < kRowBlock ? cnt - b * kRowBlock : kRowBlock;
      *reinterpret_cast<int4*>(blocks + 4 * i) = make_int4(e, first + b * kRowBlock, rows, 0);
    }
  }
  for (int i = total + e; i < nb_max; i += 256) *reinterpret_cast<int4*>(blocks + 4 * i) = make_int4(0, 0, 0, 0);
}

// ---- grouped GEMM -------------------------------------------------------------------------------------------------
enum { EPI_SILU = 0, EPI_F32 = 1 };
constexpr int kStageBytes = kRowBlock * 256;                      // [128 rows][128 k] bf16

// EPI_SILU: src = x [m, K] gathered by token, W = gate|up [E][2 * out_cols][K], out = h [P, out_cols] bf16; a workgroup
//           covers 64 columns of h (wave: gate tile + up tile).
// EPI_F32 : src = h [P, K] in sorted order, W = down [E][out_cols][K], out = y [P, out_cols] fp32; a workgroup covers
//           128 columns (wave: two neighbouring tiles).
template <int EPI, bool PACKED>
__global__ __launch_bounds__(256) void moe_gemm_kernel(const bf16_t* __restrict__ src, const bf16_t* __restrict__ w,
                                                       void* __restrict__ out, const int* __restrict__ blocks,
                                                       const int* __restrict__ sorted, int top_k, int K, int out_cols) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kStageBytes];
  const int4 blk = *reinterpret_cast<const int4*>(blocks + 4 * blockIdx.y);
  const int expert = __builtin_amdgcn_readfirstlane(blk.x);
  const int first = __builtin_amdgcn_readfirstlane(blk.y);
  const int R = __builtin_amdgcn_readfirstlane(blk.z);
  if (R <= 0) return;                                             // padded entry: the whole workgroup leaves
  const int ntiles = (R + 15) >> 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const int steps = K >> 7;

  // this thread's share of the x tile: row tile i, row i * 16 + tid / 16, 16-byte chunk tid % 16
  const int xr = tid >> 4, xc = tid & 15;
  const bf16_t* xsrc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = i * 16 + xr;
    xsrc[i] = nullptr;
    if (r < R) {
      const int64_t row = EPI == EPI_SILU ? sorted[first + r] / top_k : first + r;
      xsrc[i] = src + row * K + xc * 8;
    }
  }
  const int xdst = xr * 256 + ((xc ^ xr) << 4);

  // weight tiles of this wave
  const int n_per = EPI == EPI_SILU ? 2 * out_cols : out_cols;
  int wrow[2], col0;
  if (EPI == EPI_SILU) {
    col0 = blockIdx.x * 64 + wave * 16;
    wrow[0] = col0;
    wrow[1] = out_cols + col0;
  } else {
    col0 = blockIdx.x * 128 + wave * 32;
    wrow[0] = col0;
    wrow[1] = col0 + 16;
  }
  const bf16_t* wp[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int64_t grow = (int64_t)expert * n_per + wrow[nt];
    wp[nt] = PACKED ? w + (grow >> 4) * ((int64_t)K * 16) + lane * 8 : w + (grow + l15) * K + lq * 8;
  }
  constexpr int kWBlk = PACKED ? 512 : 32;                        // elements between consecutive 32-wide k blocks

  f32x4_t acc[8][2];
#pragma unroll
  for (int mt = 0; mt < 8; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  u32x4_t xv[8], wf[2][4], wn[2][4];
  auto xload = [&](int s) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      xv[i] = u32x4_t{0u, 0u, 0u, 0u};
      if (i < ntiles && xsrc[i]) xv[i] = *reinterpret_cast<const u32x4_t*>(xsrc[i] + s * 128);
    }
  };
  auto xstore = [&](int stage) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < ntiles) *reinterpret_cast<u32x4_t*>(smem + stage * kStageBytes + i * 16 * 256 + xdst) = xv[i];
  };
  auto wload = [&](u32x4_t (*dst)[4], int s) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
        dst[nt][kb] = *reinterpret_cast<const u32x4_t*>(wp[nt] + (int64_t)(s * 4 + kb) * kWBlk);
  };

  xload(0);
  wload(wf, 0);
  xstore(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const bool more = s + 1 < steps;
    if (more) {
      xload(s + 1);
      wload(wn, s + 1);
    }
    const unsigned char* xs = smem + (s & 1) * kStageBytes;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const int foff = l15 * 256 + (((kb * 4 + lq) ^ l15) << 4);
#pragma unroll
      for (int mt = 0; mt < 8; ++mt)
        if (mt < ntiles) {
          const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(xs + mt * 16 * 256 + foff);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wf[nt][kb]), b,
                                                                  acc[mt][nt], 0, 0, 0);
        }
    }
    if (more) {
      xstore((s + 1) & 1);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) wf[nt][kb] = wn[nt][kb];
    }
    __syncthreads();                                              // stage (s + 1) & 1 is staged, stage s & 1 is free
  }

#pragma unroll
  for (int mt = 0; mt < 8; ++mt) {
    const int r = mt * 16 + l15;
    if (mt >= ntiles || r >= R) continue;
    const int64_t orow = first + r;
    if (EPI == EPI_SILU) {
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = round_bf16(silu_f32(round_bf16(acc[mt][0][q])) * round_bf16(acc[mt][1][q]));
      const u32x2_t ov = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
      *reinterpret_cast<u32x2_t*>((bf16_t*)out + orow * out_cols + col0 + lq * 4) = ov;
    } else {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        *reinterpret_cast<f32x4_t*>((float*)out + orow * out_cols + col0 + nt * 16 + lq * 4) = acc[mt][nt];
    }
  }
}

// out[t] = bf16(sum_j w[t, j] * y[pos[t, j]]), slots in order, fp32.
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* __restrict__ y, const int* __restrict__ pos,
                                                          const float* __restrict__ wts, bf16_t* __restrict__ out,
                                                          int hidden, int top_k, int P) {
  const int64_t t = blockIdx.x;
  int p[kMaxTopK];
  float wt[kMaxTopK];
#pragma unroll
  for (int j = 0; j < kMaxTopK; ++j) {
    p[j] = -1;
    wt[j] = 0.f;
    if (j < top_k) {
      p[j] = pos[t * top_k + j];
      wt[j] = wts[t * top_k + j];
    }
  }
  for (int c = threadIdx.x * 4; c < hidden; c += 1024) {
    f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kMaxTopK; ++j)
      if (j < top_k && (unsigned)p[j] < (unsigned)P) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(y + (int64_t)p[j] * hidden + c);
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = fmaf(wt[j], v[q], a[q]);
      }
    const u32x2_t o = {pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3])};
    *reinterpret_cast<u32x2_t*>(out + t * hidden + c) = o;
  }
}

}  // namespace

void moe_launch_combine(const float* y, const int* pos, const float* topk_w, void* out, int64_t m, int hidden, int top_k,
                        int pairs, hipStream_t stream) {
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)m), dim3(256), 0, stream, y, pos, topk_w, (bf16_t*)out, hidden,
                     top_k, pairs);
}

extern "C" size_t nvl_moe_workspace_bytes(int64_t max_tokens, int hidden, int inter, int E, int top_k) {
  if (max_tokens < 1 || max_tokens > (1 << 20) || hidden < 128 || hidden % 128 || inter < 128 || inter % 128 || E < 1 ||
      E > kMaxE || top_k < 1 || top_k > kMaxTopK || top_k > E)
    return 0;
  return moe_layout(max_tokens, hidden, inter, E, top_k).total;
}

extern "C" int nvl_moe_route(const void* x, const void* router_w, int32_t* topk_ids, float* topk_w, int64_t m,
                             int hidden, int E, int top_k, int norm_topk_prob, void* stream) {
  NVL_REQUIRE(x && router_w && topk_ids && topk_w, "nvl_moe_route: null pointer");
  if (!moe_shape_ok(m, E, top_k, "nvl_moe_route")) return NVL_EINVAL;
  NVL_REQUIRE(hidden >= 128 && hidden % 128 == 0 && hidden <= 4096,
              "nvl_moe_route: hidden=%d must be a multiple of 128, at most 4096", hidden);
  NVL_REQUIRE(((uintptr_t)x | (uintptr_t)router_w) % 16 == 0, "nvl_moe_route: pointers must be 16-byte aligned");
  if (m == 0) return NVL_OK;
  const dim3 grid((unsigned)m);
  if (hidden <= 2048)
    hipLaunchKernelGGL(moe_route_kernel<4>, grid, dim3(64), 0, (hipStream_t)stream, (const bf16_t*)x,
                       (const bf16_t*)router_w, topk_ids, topk_w, m, hidden, E, top_k, norm_topk_prob);
  else
    hipLaunchKernelGGL(moe_route_kernel<8>, grid, dim3(64), 0, (hipStream_t)stream, (const bf16_t*)x,
                       (const bf16_t*)router_w, topk_ids, topk_w, m, hidden, E, top_k, norm_topk_prob);
  return nvl_check_launch("nvl_moe_route");
}

extern "C" int nvl_moe_plan(const int32_t* topk_ids, int64_t m, int E, int top_k, void* workspace,
                            size_t workspace_bytes, void* stream) {
  NVL_REQUIRE(topk_ids && workspace, "nvl_moe_plan: null pointer");
  if (!moe_shape_ok(m, E, top_k, "nvl_moe_plan")) return NVL_EINVAL;
  NVL_REQUIRE((uintptr_t)workspace % 256 == 0, "nvl_moe_plan: workspace must be 256-byte aligned");
  const MoeLayout l = moe_layout(m, 128, 128, E, top_k);
  NVL_REQUIRE(l.index_end <= workspace_bytes,
              "nvl_moe_plan: m=%lld tokens are above the cap of this workspace (%zu bytes; nvl_moe_workspace_bytes)",
              (long long)m, workspace_bytes);
  if (m == 0) return NVL_OK;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(moe_sort_kernel, dim3((unsigned)E), dim3(256), 0, (hipStream_t)stream, topk_ids, (int)l.pairs, E,
                     (int*)(ws + l.offsets), (int*)(ws + l.sorted), (int*)(ws + l.pos));
  hipLaunchKernelGGL(moe_blocks_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)(ws + l.offsets), E,
                     (int*)(ws + l.blocks), (int)l.nb_max);
  return nvl_check_launch("nvl_moe_plan");
}

extern "C" int nvl_moe_experts(const void* x, const void* w_gate_up, const void* w_down, const int32_t* topk_ids,
                               const float* topk_w, void* out, int64_t m, int hidden, int inter, int E, int top_k,
                               int weight_layout, void* workspace, size_t workspace_bytes, void* stream) {
  NVL_REQUIRE(x && w_gate_up && w_down && topk_ids && topk_w && out && workspace, "nvl_moe_experts: null pointer");
  if (!moe_shape_ok(m, E, top_k, "nvl_moe_experts")) return NVL_EINVAL;
  NVL_REQUIRE(hidden >= 128 && hidden % 128 == 0, "nvl_moe_experts: hidden=%d must be a multiple of 128", hidden);
  NVL_REQUIRE(inter >= 128 && inter % 128 == 0, "nvl_moe_experts: inter=%d must be a multiple of 128", inter);
  NVL_REQUIRE(weight_layout == 0 || weight_layout == 1, "nvl_moe_experts: weight_layout must be 0 or 1");
  NVL_REQUIRE(((uintptr_t)x | (uintptr_t)w_gate_up | (uintptr_t)w_down | (uintptr_t)out) % 16 == 0 &&
                  (uintptr_t)workspace % 256 == 0,
              "nvl_moe_experts: pointers must be 16-byte aligned (workspace: 256)");
  const MoeLayout l = moe_layout(m, hidden, inter, E, top_k);
  NVL_REQUIRE(l.total <= workspace_bytes,
              "nvl_moe_experts: m=%lld tokens are above the cap of this workspace (%zu bytes; nvl_moe_workspace_bytes)",
              (long long)m, workspace_bytes);
  NVL_REQUIRE(l.nb_max <= 65535, "nvl_moe_experts: too many row blocks (%lld)", (long long)l.nb_max);
  if (m == 0) return NVL_OK;
  char* ws = (char*)workspace;
  const int* blocks = (const int*)(ws + l.blocks);
  const int* sorted = (const int*)(ws + l.sorted);
  bf16_t* h = (bf16_t*)(ws + l.h);
  float* y = (float*)(ws + l.y);
  const dim3 g1((unsigned)(inter / 64), (unsigned)l.nb_max), g2((unsigned)(hidden / 128), (unsigned)l.nb_max);
  hipStream_t st = (hipStream_t)stream;
  if (weight_layout == 1) {
    hipLaunchKernelGGL((moe_gemm_kernel<EPI_SILU, true>), g1, dim3(256), 0, st, (const bf16_t*)x,
                       (const bf16_t*)w_gate_up, (void*)h, blocks, sorted, top_k, hidden, inter);
    hipLaunchKernelGGL((moe_gemm_kernel<EPI_F32, true>), g2, dim3(256), 0, st, (const bf16_t*)h, (const bf16_t*)w_down,
                       (void*)y, blocks, sorted, top_k, inter, hidden);
  } else {
    hipLaunchKernelGGL((moe_gemm_kernel<EPI_SILU, false>), g1, dim3(256), 0, st, (const bf16_t*)x,
                       (const bf16_t*)w_gate_up, (void*)h, blocks, sorted, top_k, hidden, inter);
    hipLaunchKernelGGL((moe_gemm_kernel<EPI_F32, false>), g2, dim3(256), 0, st, (const bf16_t*)h, (const bf16_t*)w_down,
                       (void*)y, blocks, sorted, top_k, inter, hidden);
  }
  moe_launch_combine(y, (const int*)(ws + l.pos), topk_w, out, m, hidden, top_k, (int)l.pairs, st);
  return nvl_check_launch("nvl_moe_experts");
}
