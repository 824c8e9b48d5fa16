// MXFP4 expert weights for the Qwen3-MoE block (LLM(path, weight_dtype="mxfp4")): the quantiser / packer and the grouped
// expert GEMMs over 4-bit weights. Routing, the plan, the workspace and the combine are moe.hip's, unchanged.
//
// Format (OCP microscaling): element e2m1 — codes 0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6, bit 3 the sign — and one e8m0 scale
// byte s (2^(s - 127)) per row and 32 consecutive k: exactly the K of one v_mfma_f32_16x16x32_bf16, so one scale covers
// one A fragment. Per block, with A = max |w|: A = 0 -> byte 127, codes 0; else E = floor(log2 A) - 2 (from the bf16
// exponent field; clamped to >= -126, so byte 0 never occurs), byte E + 127, element = w / 2^E (exact) rounded to the
// nearest code magnitude, ties to the even code, above 6 saturating to 6. The block maximum lands on 4 or 6, so
// quantising a dequantised matrix again reproduces it.
//
// Storage of a stacked [N = E * n, K] matrix:
//   codes  [N/16][K/128][64 lanes][16 bytes], lane = 16 lq + l15: byte 4 kb + b of a lane holds row 16 tile + l15,
//          k = 128 step + 32 kb + 8 lq + 2 b (low nibble) and that k + 1 (high nibble) — dword kb of a lane is its whole
//          A fragment of k block kb, a wave load of a tile's k step is one contiguous KiB;
//   scales [N][K/32] bytes, row-major: lane (l15, .) reads its row's four scales of a k step as one dword.
//
//   nvl_quant_pack_mxfp4  one wave per (16-row tile, 128-wide k step), one pass over the bf16 matrix: lane (l15, lq)
//                         loads its four 16-byte fragments, the block maximum is a max over the four lq lanes of a row
//                         (two cross-lane exchanges on the bf16 bit patterns), codes come from seven compares against
//                         the rounding boundaries. No fp32 image of the matrix exists.
//   nvl_moe_experts_mxfp4 (a) gate|up + SiLU * mul, (b) down, (c) moe.hip's combine: nvl_moe_experts' three launches and
//                         rounding points. The GEMM keeps moe_gemm_kernel's row-block staging (<= 128 gathered rows per
//                         128-wide k step in LDS, XOR swizzle, two stages, one barrier per step) and changes the weight
//                         side: a lane's A fragments of a tile's k step arrive as ONE 16-byte load of codes plus one
//                         dword of scales, one step ahead, and are expanded in registers — v_cvt_scalef32_pk_bf16_fp4,
//                         four per fragment, each turning one byte (two codes) and the block scale into two bf16.
//   Work split: FOUR 16-column tiles per wave (bf16 kernel: two). A 4-bit tile step is 1 KiB where a bf16 one is 4; with
//   two tiles a wave would move 2 KiB behind the same barrier, LDS stage and load latency that already bound the bf16
//   kernel. A workgroup therefore covers 128 h columns in (a) — per wave two gate tiles and THEIR two up tiles — and 256
//   y columns in (b) — four neighbouring tiles — which also halves the x re-gather per weight byte. That is 128
//   accumulator registers at 8 row tiles; 256 threads at one wave per SIMD have 512. hidden % 256 == 128: the last
//   workgroup of (b) runs two tiles per wave (a workgroup-uniform count, the other two are never loaded or multiplied).
//   Padded row blocks leave before the first barrier.
#include "moe_common.h"

namespace {

constexpr int kStageBytes = kRowBlock * 256;                      // [128 rows][128 k] bf16
constexpr int kTiles = 4;                                         // 16-column weight tiles per wave
enum { EPI_SILU = 0, EPI_F32 = 1 };

__device__ __forceinline__ float e8m0_to_f32(unsigned int byte) { return __uint_as_float(byte << 23); }

// 8 codes (one dword: nibble j = element j) x scale -> the 8 bf16 of an MFMA A fragment. Operand byte `sel`, low nibble
// first.
__device__ __forceinline__ bf16x8_t expand_fp4x8(unsigned int c, float scale) {
  u32x4_t r;
  r[0] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 0));
  r[1] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 1));
  r[2] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 2));
  r[3] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 3));
  return __builtin_bit_cast(bf16x8_t, r);
}

// ---- quantise + pack ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moe_quant_pack_mxfp4_kernel(const bf16_t* __restrict__ w, int64_t items, int ksteps,
                                                                   int64_t K, unsigned char* __restrict__ codes,
                                                                   unsigned char* __restrict__ scales) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // (tile, k step), k steps fastest
  if (item >= items) return;
  const int64_t tile = item / ksteps;
  const int s = (int)(item - tile * ksteps);
  const int64_t row = tile * 16 + l15;
  const bf16_t* src = w + row * K + s * 128 + lq * 8;
  u32x4_t v[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) v[kb] = *reinterpret_cast<const u32x4_t*>(src + kb * 32);
  u32x4_t out;
  unsigned int sbytes = 0;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    // block maximum on the bit patterns (|bf16| is monotone in its 15 low bits): this lane's 8, then the row's 4 lanes
    unsigned int mx = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned int lo = v[kb][i] & 0x7fffu, hi = (v[kb][i] >> 16) & 0x7fffu;
      mx = mx > lo ? mx : lo;
      mx = mx > hi ? mx : hi;
    }
    unsigned int o = (unsigned int)__shfl_xor((int)mx, 16, 64);
    mx = mx > o ? mx : o;
    o = (unsigned int)__shfl_xor((int)mx, 32, 64);
    mx = mx > o ? mx : o;
    const int ea = (int)(mx >> 7);                                  // biased exponent of A: floor(log2 A) + 127
    const int sb = mx == 0 ? 127 : (ea - 2 > 1 ? ea - 2 : 1);       // scale byte E + 127, E clamped to >= -126
    const float inv = __uint_as_float((unsigned int)(254 - sb) << 23);    // 2^-E
    unsigned int c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned int bits = (j & 1) ? v[kb][j >> 1] >> 16 : v[kb][j >> 1] & 0xffffu;
      const float f = __uint_as_float((bits & 0x7fffu) << 16) * inv;      // |w| / 2^E: exact, < 8
      // boundaries between the code magnitudes; a tie goes to the even code: > where the lower code is even
      unsigned int q = (f > 0.25f) + (f >= 0.75f) + (f > 1.25f) + (f >= 1.75f) + (f > 2.5f) + (f >= 3.5f) + (f > 5.f);
      if (bits > 0x8000u) q |= 8u;                                  // w < 0 (-0 stays code 0)
      c |= q << (4 * j);
    }
    out[kb] = c;
    sbytes |= (unsigned int)sb << (8 * kb);
  }
  *reinterpret_cast<u32x4_t*>(codes + (item * 64 + lane) * 16) = out;
  if (lq == 0) *reinterpret_cast<unsigned int*>(scales + row * (K >> 5) + s * 4) = sbytes;
}

// ---- grouped GEMM over 4-bit weights ------------------------------------------------------------------------------
// EPI_SILU: src = x [m, K] gathered by token, W = gate|up [E][2 * out_cols][K], out = h [P, out_cols] bf16; a workgroup
//           covers 128 columns of h (wave: gate tiles c, c + 16 and up tiles c, c + 16; acc[.][j] pairs with acc[.][2 + j]).
// EPI_F32 : src = h [P, K] in sorted order, W = down [E][out_cols][K], out = y [P, out_cols] fp32; a workgroup covers 256
//           columns (wave: four neighbouring tiles), the last one 128 when out_cols % 256 == 128 (wave: two).
template <int EPI>
__global__ __launch_bounds__(256) void moe_gemm_mxfp4_kernel(const bf16_t* __restrict__ src,
                                                             const unsigned char* __restrict__ codes,
                                                             const unsigned char* __restrict__ scales,
                                                             void* __restrict__ out, const int* __restrict__ blocks,
                                                             const int* __restrict__ sorted, int top_k, int K,
                                                             int out_cols) {
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

  // weight tiles of this wave: rows wrow[nt] ... + 15 of the expert's matrix, nt < ntv
  const int n_per = EPI == EPI_SILU ? 2 * out_cols : out_cols;
  int wrow[kTiles], col0, ntv = kTiles;
  if (EPI == EPI_SILU) {
    col0 = blockIdx.x * 128 + wave * 32;
    wrow[0] = col0;
    wrow[1] = col0 + 16;
    wrow[2] = out_cols + col0;
    wrow[3] = out_cols + col0 + 16;
  } else {
    const bool tail = (int)(blockIdx.x + 1) * 256 > out_cols;     // 128 columns left: two tiles per wave
    ntv = tail ? 2 : kTiles;
    col0 = blockIdx.x * 256 + wave * (tail ? 32 : 64);
#pragma unroll
    for (int nt = 0; nt < kTiles; ++nt) wrow[nt] = col0 + nt * 16;
  }
  const unsigned char* cp[kTiles];
  const unsigned char* sp[kTiles];
#pragma unroll
  for (int nt = 0; nt < kTiles; ++nt) {
    const int64_t grow = (int64_t)expert * n_per + (nt < ntv ? wrow[nt] : wrow[0]);
    cp[nt] = codes + (grow >> 4) * ((int64_t)steps * 1024) + lane * 16;
    sp[nt] = scales + (grow + l15) * (int64_t)(K >> 5);
  }

  f32x4_t acc[8][kTiles];
#pragma unroll
  for (int mt = 0; mt < 8; ++mt)
#pragma unroll
    for (int nt = 0; nt < kTiles; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  u32x4_t xv[8], wf[kTiles], wn[kTiles];
  unsigned int sf[kTiles], sn[kTiles];
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
  auto wload = [&](u32x4_t* dst, unsigned int* sdst, int s) {
#pragma unroll
    for (int nt = 0; nt < kTiles; ++nt)
      if (nt < ntv) {
        dst[nt] = *reinterpret_cast<const u32x4_t*>(cp[nt] + (int64_t)s * 1024);
        sdst[nt] = *reinterpret_cast<const unsigned int*>(sp[nt] + s * 4);
      }
  };

  xload(0);
  wload(wf, sf, 0);
  xstore(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const bool more = s + 1 < steps;
    if (more) {
      xload(s + 1);
      wload(wn, sn, s + 1);
    }
    const unsigned char* xs = smem + (s & 1) * kStageBytes;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      bf16x8_t a[kTiles];
#pragma unroll
      for (int nt = 0; nt < kTiles; ++nt)
        if (nt < ntv) a[nt] = expand_fp4x8(wf[nt][kb], e8m0_to_f32((sf[nt] >> (8 * kb)) & 0xffu));
      const int foff = l15 * 256 + (((kb * 4 + lq) ^ l15) << 4);
#pragma unroll
      for (int mt = 0; mt < 8; ++mt)
        if (mt < ntiles) {
          const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(xs + mt * 16 * 256 + foff);
#pragma unroll
          for (int nt = 0; nt < kTiles; ++nt)
            if (nt < ntv) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt], b, acc[mt][nt], 0, 0, 0);
        }
    }
    if (more) {
      xstore((s + 1) & 1);
#pragma unroll
      for (int nt = 0; nt < kTiles; ++nt) {
        wf[nt] = wn[nt];
        sf[nt] = sn[nt];
      }
    }
    __syncthreads();                                              // stage (s + 1) & 1 is staged, stage s & 1 is free
  }

#pragma unroll
  for (int mt = 0; mt < 8; ++mt) {
    const int r = mt * 16 + l15;
    if (mt >= ntiles || r >= R) continue;
    const int64_t orow = first + r;
    if (EPI == EPI_SILU) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          o[q] = round_bf16(silu_f32(round_bf16(acc[mt][j][q])) * round_bf16(acc[mt][2 + j][q]));
        const u32x2_t ov = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
        *reinterpret_cast<u32x2_t*>((bf16_t*)out + orow * out_cols + col0 + j * 16 + lq * 4) = ov;
      }
    } else {
#pragma unroll
      for (int nt = 0; nt < kTiles; ++nt)
        if (nt < ntv) *reinterpret_cast<f32x4_t*>((float*)out + orow * out_cols + col0 + nt * 16 + lq * 4) = acc[mt][nt];
    }
  }
}

}  // namespace

extern "C" int nvl_quant_pack_mxfp4(const void* w_bf16, int64_t n, int64_t k, void* codes_out, void* scales_out,
                                    void* stream) {
  NVL_REQUIRE(w_bf16 && codes_out && scales_out, "nvl_quant_pack_mxfp4: null pointer");
  NVL_REQUIRE(n > 0 && n % 16 == 0, "nvl_quant_pack_mxfp4: n=%lld must be a positive multiple of 16", (long long)n);
  NVL_REQUIRE(k > 0 && k % 128 == 0, "nvl_quant_pack_mxfp4: k=%lld must be a positive multiple of 128", (long long)k);
  NVL_REQUIRE(((uintptr_t)w_bf16 | (uintptr_t)codes_out | (uintptr_t)scales_out) % 16 == 0,
              "nvl_quant_pack_mxfp4: pointers must be 16-byte aligned");
  const int64_t items = (n / 16) * (k / 128);
  NVL_REQUIRE(k / 128 <= (1 << 20) && (items + 3) / 4 <= 0x7fffffffLL,
              "nvl_quant_pack_mxfp4: n=%lld k=%lld is too large for one launch", (long long)n, (long long)k);
  hipLaunchKernelGGL(moe_quant_pack_mxfp4_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)w_bf16, items, (int)(k / 128), k, (unsigned char*)codes_out,
                     (unsigned char*)scales_out);
  return nvl_check_launch("nvl_quant_pack_mxfp4");
}

extern "C" int nvl_moe_experts_mxfp4(const void* x, const void* gu_codes, const void* gu_scales, const void* dn_codes,
                                     const void* dn_scales, const int32_t* topk_ids, const float* topk_w, void* out,
                                     int64_t m, int hidden, int inter, int E, int top_k, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  NVL_REQUIRE(x && gu_codes && gu_scales && dn_codes && dn_scales && topk_ids && topk_w && out && workspace,
              "nvl_moe_experts_mxfp4: null pointer");
  if (!moe_shape_ok(m, E, top_k, "nvl_moe_experts_mxfp4")) return NVL_EINVAL;
  NVL_REQUIRE(hidden >= 128 && hidden % 128 == 0, "nvl_moe_experts_mxfp4: hidden=%d must be a multiple of 128", hidden);
  NVL_REQUIRE(inter >= 128 && inter % 128 == 0, "nvl_moe_experts_mxfp4: inter=%d must be a multiple of 128", inter);
  NVL_REQUIRE(((uintptr_t)x | (uintptr_t)gu_codes | (uintptr_t)gu_scales | (uintptr_t)dn_codes | (uintptr_t)dn_scales |
               (uintptr_t)out) % 16 == 0 && (uintptr_t)workspace % 256 == 0,
              "nvl_moe_experts_mxfp4: pointers must be 16-byte aligned (workspace: 256)");
  const MoeLayout l = moe_layout(m, hidden, inter, E, top_k);
  NVL_REQUIRE(l.total <= workspace_bytes,
              "nvl_moe_experts_mxfp4: m=%lld tokens are above the cap of this workspace (%zu bytes; nvl_moe_workspace_bytes)",
              (long long)m, workspace_bytes);
  NVL_REQUIRE(l.nb_max <= 65535, "nvl_moe_experts_mxfp4: too many row blocks (%lld)", (long long)l.nb_max);
  if (m == 0) return NVL_OK;
  char* ws = (char*)workspace;
  const int* blocks = (const int*)(ws + l.blocks);
  const int* sorted = (const int*)(ws + l.sorted);
  bf16_t* h = (bf16_t*)(ws + l.h);
  float* y = (float*)(ws + l.y);
  const dim3 g1((unsigned)(inter / 128), (unsigned)l.nb_max), g2((unsigned)((hidden + 255) / 256), (unsigned)l.nb_max);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((moe_gemm_mxfp4_kernel<EPI_SILU>), g1, dim3(256), 0, st, (const bf16_t*)x,
                     (const unsigned char*)gu_codes, (const unsigned char*)gu_scales, (void*)h, blocks, sorted, top_k,
                     hidden, inter);
  hipLaunchKernelGGL((moe_gemm_mxfp4_kernel<EPI_F32>), g2, dim3(256), 0, st, (const bf16_t*)h,
                     (const unsigned char*)dn_codes, (const unsigned char*)dn_scales, (void*)y, blocks, sorted, top_k,
                     inter, hidden);
  moe_launch_combine(y, (const int*)(ws + l.pos), topk_w, out, m, hidden, top_k, (int)l.pairs, st);
  return nvl_check_launch("nvl_moe_experts_mxfp4");
}
