// Weight-only FP8 (W8A16) TILE linear for gfx950, any row count:
//   out[M, N] = x[M, K] (bf16) . (W8[N, K] (OCP e4m3) o S)^T,  S fp32 POWERS OF TWO, one per (16-row weight tile, 128-column k block)
// on the packed tiles and scales nvl_linear_wide_fp8 streams (nvl_pack_weight_tiles_fp8: no second layout, no second copy).
// It serves what that kernel's plan refuses — every M > 256 (prefill, decode batches of 257-512 sequences) — so that
// weight_dtype="fp8_only" can release the bf16 parameter the library GEMM needed.
//
// Semantics. The weight enters the matrix instruction as bf16(w8 x s): v_cvt_scalef32_pk_bf16_fp8 with the block's scale.
// For a power-of-two s with w8 x s a normal bf16 (what LinearBase._pack_fp8 produces) that is exact, so the result is
// x . W_deq^T with fp32 accumulation — the matrix weight_dtype="fp8" multiplies in prefill, in another summation order.
// There is no per-block second accumulator: arbitrary fp32 scales are nvl_linear_wide_fp8's contract, not this one's.
//
// Decomposition. Above 256 rows the GEMM is bound by the matrix pipe, not by the weight stream (512 rows of the 8B gate|up:
// ~0.1 ms of MFMA against ~0.02 ms of weight bytes), so gemm_wide's "every row of a row group in one wave" does not carry
// over; this is an output-tiled kernel:
//   * workgroup = 4 consumer waves (2 x 2) + 1 loader wave. It owns BM x BN outputs — 256 x 128 (MT = 8 row tiles x NT = 4
//     column tiles per wave, 128 fp32 accumulator registers) or, where that grid would leave CUs idle, 128 x 64 (MT = 4,
//     NT = 2) — and walks K in 64-column steps: one packed fragment pair (1 KiB) per column tile and step.
//   * x operand: the loader wave stages x[BM, 64] (128 B per row) two steps ahead into three LDS stages by LDS-DMA
//     (global_load_lds_dwordx4, 8 rows per instruction); slot c of row r holds 16-byte chunk c ^ (r & 7), so the 16 rows a
//     ds_read_b128 fragment read touches spread over all banks. One barrier per step. Rows past M read row M - 1 and are
//     never stored.
//   * weight operand: global -> VGPR by the waves that own the columns (the two waves of a column half read the same KiB;
//     the second read hits the CU's vector cache), raw fp8 in a ring RING steps deep, re-requested as soon as a slot is
//     converted. The tile's scale of the step rides in the same slot (one broadcast dword, fetched with the weights, never
//     inside the MFMA chain); conversion = 4 packed converts per 8 values, once per step, shared by the MT row tiles.
//   * per step a wave issues MT x NT x 2 MFMAs (v_mfma_f32_16x16x32_bf16) on NT x MT independent chains; the x fragments
//     of row tile mt + 1 are read from LDS under the MFMAs of row tile mt.
//   * workgroup order: row blocks are the fast index inside bands of 8, so the workgroups in flight share a few weight
//     column groups AND a few x row blocks through L2.
//   * epilogue: bf16, 8-byte stores (a lane holds 4 consecutive columns of one row). SiLU: a wave's column tiles 2 j / 2 j + 1
//     are a gate tile and its up tile; the GEMM output is rounded to bf16 before the activation (nvl_linear_wide mode 1).
// Enqueue-only, no workspace: capturable. The 256 x 128 shape needs 96 KiB of LDS, opted into with hipFuncSetAttribute on
// the FIRST call of the entry on a device (whichever shape that call takes) — that call must precede the first graph
// capture; the engine's warm-up prefill is it.
#include "common.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>

namespace {

constexpr int kBK = 64;                  // k per step: one packed fragment pair
constexpr int kNS = 3;                   // x stages in LDS (the loader runs two steps ahead)
constexpr int kRowB = kBK * 2;           // bytes of one x row per step
constexpr int kRing = 2;                 // raw weight fragments in flight per wave, in steps
enum { EPI_BF16 = 0, EPI_SILU = 1 };

__device__ __forceinline__ float silu_f32(float g) { return g / (1.f + __expf(-g)); }

// 8 fp8 (two dwords) x scale -> 8 bf16 in MFMA operand order (element e = byte e)
__device__ __forceinline__ bf16x8_t fp8x8_to_bf16x8(unsigned lo, unsigned hi, float s) {
  u32x4_t r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, s, false));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, s, true));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, s, false));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, s, true));
  return __builtin_bit_cast(bf16x8_t, r);
}

template <int MT, int NT>
__global__ __launch_bounds__(5 * 64) void linear_tile_fp8_kernel(const bf16_t* __restrict__ x,
                                                                 const unsigned char* __restrict__ w8,
                                                                 const float* __restrict__ scales,
                                                                 bf16_t* __restrict__ out, int64_t M, int N, int K, int epi,
                                                                 int row_blocks, int col_groups) {
  constexpr int kRows = 2 * MT * 16;                              // BM
  constexpr int kStage = kRows * kRowB;                           // bytes per LDS stage
  constexpr int AHEAD = kNS - 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  // workgroup id -> (row block, column group): row blocks fastest inside bands of 8 row blocks
  const int band_wgs = 8 * col_groups;
  const int band = (int)blockIdx.x / band_wgs, rem = (int)blockIdx.x - band * band_wgs;
  const int band_rows = row_blocks - band * 8 < 8 ? row_blocks - band * 8 : 8;
  const int cgroup = rem / band_rows;
  const int64_t m_base = (int64_t)(band * 8 + rem - cgroup * band_rows) * kRows;
  const bool silu = epi == EPI_SILU;
  const int out_cols = silu ? N / 2 : N;
  const int steps = K / kBK, last = steps - 1;
  auto kstep = [&](int s) { return s < last ? s : last; };        // prefetches past the end re-read the last step

  if (wave >= 4) {
    // ---- loader wave: x tile of step s + 2 -> LDS stage (s + 2) % 3 by LDS-DMA ----------------------------------------------
    // instruction i covers rows 8 i + (lane >> 3), 16-byte slots lane & 7; slot c of row r holds chunk c ^ (r & 7)
    constexpr int kLC = kRows / 8;                                // 1-KiB pieces of a tile
    static_assert(kLC * (AHEAD - 1) < 64, "vmcnt is a 6-bit counter");
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const bf16_t* x_src[kLC];
#pragma unroll
    for (int i = 0; i < kLC; ++i) {
      const int row = 8 * i + (lane >> 3);
      int64_t grow = m_base + row;
      grow = grow < M ? grow : M - 1;                             // padding rows read a valid row (never stored)
      x_src[i] = x + grow * K + (((lane & 7) ^ (row & 7)) << 3);
    }
    auto issue = [&](int s) {
      const unsigned dst = lds0 + (unsigned)(s % kNS) * kStage;
      const int koff = kstep(s) * kBK;
#pragma unroll
      for (int i = 0; i < kLC; ++i) {
        unsigned keep;
        const unsigned d = __builtin_amdgcn_readfirstlane(dst + i * 1024);
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(x_src[i] + koff), "s"(d)
                     : "memory");
      }
    };
    if (steps >= AHEAD) {
#pragma unroll
      for (int a = 0; a < AHEAD; ++a) issue(a);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kLC * (AHEAD - 1)) : "memory");   // step 0 has landed
    } else {
      for (int a = 0; a < steps; ++a) issue(a);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    for (int s = 0; s < steps; ++s) {
      // stage (s + AHEAD) % 3 was last read during step s - 1: free since the previous barrier
      if (s + AHEAD <= last) {
        issue(s + AHEAD);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kLC * (AHEAD - 1)) : "memory");  // steps up to s + 1 have landed
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
    }
    return;
  }

  // ---- consumer waves: wave = 2 wr + wc owns rows [wr MT 16, ...) x column tiles (2 cgroup + wc) NT ... ----------------------
  const int wr = wave >> 1, wc = wave & 1;
  const int ntiles = out_cols >> 4;                               // output column tiles (SiLU: gate / up pairs)
  const int ksc = K / 128;                                        // scales per tile
  const int unit0 = (cgroup * 2 + wc) * (silu ? NT / 2 : NT);     // first output tile of this wave
  const unsigned char* wrow[NT];                                  // lane's 16 bytes of (tile nt, k step 0)
  const float* srow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    int tile = unit0 + (silu ? nt >> 1 : nt);
    tile = tile < ntiles ? tile : ntiles - 1;                     // ragged last column group: any valid tile, masked at the store
    if (silu && (nt & 1)) tile += ntiles;                         // the up tile of that gate tile
    wrow[nt] = w8 + (int64_t)tile * 16 * K + lane * 16;
    srow[nt] = scales + (int64_t)tile * ksc;
  }
  int frag_off[2];                                                // B fragment of k block kb: row l15 of a row tile
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) frag_off[kb] = wr * MT * 16 * kRowB + l15 * kRowB + (((kb * 4 + lq) ^ (l15 & 7)) << 4);

  f32x4_t acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  u32x4_t wf[kRing][NT];                                          // raw fp8 fragment pairs, kRing steps in flight
  float sc[kRing][NT];
  auto wload = [&](u32x4_t* dst, float* sdst, int s) {
    const int ks = kstep(s);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      dst[nt] = *reinterpret_cast<const u32x4_t*>(wrow[nt] + (int64_t)ks * 1024);
      sdst[nt] = srow[nt][ks >> 1];
    }
  };

  // one k step on ring slot (wfs, scs) and LDS stage xs; LOAD: the slot is re-requested for logical step sl as soon as its
  // fragments are converted
  auto compute = [&](auto load_tag, const unsigned char* xs, u32x4_t* wfs, float* scs, int sl) {
    constexpr bool LOAD = decltype(load_tag)::value;
    __builtin_amdgcn_sched_barrier(0);                             // (conversions stay inside their step)
    bf16x8_t a[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      a[nt][0] = fp8x8_to_bf16x8(wfs[nt][0], wfs[nt][1], scs[nt]);
      a[nt][1] = fp8x8_to_bf16x8(wfs[nt][2], wfs[nt][3], scs[nt]);
    }
    if constexpr (LOAD) wload(wfs, scs, sl);
    u32x4_t f[2][2];
    auto fread = [&](int mt, u32x4_t* dst) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) dst[kb] = *reinterpret_cast<const u32x4_t*>(xs + mt * 16 * kRowB + frag_off[kb]);
    };
    fread(0, f[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      if (mt + 1 < MT) fread(mt + 1, f[(mt + 1) & 1]);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)                            // NT independent chains, interleaved
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt][kb], __builtin_bit_cast(bf16x8_t, f[mt & 1][kb]),
                                                                acc[mt][nt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);                           // (keeps the reads of row tile mt + 2 out of this one)
    }
  };

  // Pipeline invariant at the top of step s (slot i = s mod kRing): LDS stage s % 3 holds x of step s, slots i .. i + kRing - 1
  // hold (or have in flight) the weights and scales of steps s .. s + kRing - 1.
#pragma unroll
  for (int r = 0; r < kRing; ++r) wload(wf[r], sc[r], r);
  __syncthreads();                                                // stage 0 is staged
  const int nblk = steps / kRing;
  for (int blk = 0; blk < nblk; ++blk) {
#pragma unroll
    for (int i = 0; i < kRing; ++i) {
      const int s = blk * kRing + i;
      compute(std::true_type{}, smem + (s % kNS) * kStage, wf[i], sc[i], s + kRing);
      __syncthreads();                                            // stage (s + 1) % 3 is staged, stage s % 3 is free
    }
  }
#pragma unroll
  for (int i = 0; i < kRing - 1; ++i) {
    const int s = nblk * kRing + i;
    if (s < steps) {
      compute(std::false_type{}, smem + (s % kNS) * kStage, wf[i], sc[i], 0);
      __syncthreads();
    }
  }

  // ---- epilogue: lane (l15, lq) holds out[row = 16 mt + l15][col = 16 tile + 4 lq .. + 3] ---------------------------------
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int64_t m = m_base + (wr * MT + mt) * 16 + l15;
    if (m >= M) continue;
    bf16_t* orow = out + m * out_cols + lq * 4;
    if (silu) {
#pragma unroll
      for (int j = 0; j < NT / 2; ++j) {
        if (unit0 + j >= ntiles) continue;
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = silu_f32(round_bf16(acc[mt][2 * j][r])) * round_bf16(acc[mt][2 * j + 1][r]);
        u32x2_t ov = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
        *reinterpret_cast<u32x2_t*>(orow + (unit0 + j) * 16) = ov;
      }
    } else {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if (unit0 + nt >= ntiles) continue;
        u32x2_t o = {pack_bf16x2(acc[mt][nt][0], acc[mt][nt][1]), pack_bf16x2(acc[mt][nt][2], acc[mt][nt][3])};
        *reinterpret_cast<u32x2_t*>(orow + (unit0 + nt) * 16) = o;
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
template <int MT, int NT>
constexpr size_t tile_lds() { return (size_t)kNS * 2 * MT * 16 * kRowB; }

template <int MT, int NT>
int launch_tile(const void* x, const void* w8, const void* scales, void* out, int64_t m, int n, int k, int epi, hipStream_t s) {
  const int64_t row_blocks = (m + 2 * MT * 16 - 1) / (2 * MT * 16);
  const int units = (epi == EPI_SILU ? n / 2 : n) / 16, per = 2 * (epi == EPI_SILU ? NT / 2 : NT);
  const int col_groups = (units + per - 1) / per;
  NVL_REQUIRE(row_blocks * col_groups < (1ll << 31), "nvl_linear_tile_fp8: m=%lld n=%d: grid too large", (long long)m, n);
  hipLaunchKernelGGL((linear_tile_fp8_kernel<MT, NT>), dim3((unsigned)(row_blocks * col_groups)), dim3(5 * 64), (tile_lds<MT, NT>()),
                     s, (const bf16_t*)x, (const unsigned char*)w8, (const float*)scales, (bf16_t*)out, m, n, k, epi,
                     (int)row_blocks, col_groups);
  return nvl_check_launch("nvl_linear_tile_fp8");
}

}  // namespace

extern "C" int nvl_linear_tile_fp8(const void* x, const void* w8_packed, const void* scales, void* out, int64_t m, int n, int k,
                                   int mode, void* stream) {
  NVL_REQUIRE(x && w8_packed && scales && out, "nvl_linear_tile_fp8: null pointer");
  NVL_REQUIRE(mode >= 0 && mode <= 2, "nvl_linear_tile_fp8: mode=%d (0 bf16, 1 silu*mul)", mode);
  if (mode == 2) {
    nvl_set_error("nvl_linear_tile_fp8: mode 2 (split-K fp32 partials) is not offered at these sizes: take mode 0");
    return NVL_EUNSUPPORTED;
  }
  NVL_REQUIRE(m >= 1 && k >= 128 && k % 128 == 0, "nvl_linear_tile_fp8: m=%lld must be >= 1, k=%d a multiple of 128", (long long)m, k);
  NVL_REQUIRE(n >= 16 && n % (mode == EPI_SILU ? 32 : 16) == 0, "nvl_linear_tile_fp8: n=%d must be a multiple of %d", n,
              mode == EPI_SILU ? 32 : 16);
  NVL_REQUIRE(((uintptr_t)x | (uintptr_t)w8_packed | (uintptr_t)out) % 16 == 0 && (uintptr_t)scales % 4 == 0,
              "nvl_linear_tile_fp8: pointers must be 16-byte aligned (scales: 4)");
  // 96 KiB of LDS for the 256 x 128 shape: opted into on the first call per device, whichever shape it takes, so that the
  // call is behind us before any graph capture (the engine's warm-up prefill; hipFuncSetAttribute is not a stream operation)
  static bool attr_done[NVL_MAX_DEVICES] = {};
  bool& attr_set = attr_done[nvl_device_slot()];
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&linear_tile_fp8_kernel<8, 4>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)tile_lds<8, 4>()) != hipSuccess) {
      nvl_set_error("nvl_linear_tile_fp8: cannot reserve %zu B of LDS", tile_lds<8, 4>());
      return NVL_ELAUNCH;
    }
    attr_set = true;
  }
  // Tile shape: 256 x 128 where that grid gives every CU a workgroup, else 128 x 64 (4 x the workgroups).
  // NVL_TILE_FP8=big|small forces one (A/B measurements; the only switch of this kernel).
  const int out_cols = mode == EPI_SILU ? n / 2 : n;
  bool big = ((m + 255) / 256) * ((out_cols + 127) / 128) >= nvl_device_cu_count();
  if (const char* e = getenv("NVL_TILE_FP8")) big = !strcmp(e, "big") ? true : !strcmp(e, "small") ? false : big;
  hipStream_t s = (hipStream_t)stream;
  return big ? launch_tile<8, 4>(x, w8_packed, scales, out, m, n, k, mode, s)
             : launch_tile<4, 2>(x, w8_packed, scales, out, m, n, k, mode, s);
}
