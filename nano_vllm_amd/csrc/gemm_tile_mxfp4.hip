// Weight-only MXFP4 (W4A16) TILE linear for gfx950, any row count (LLM(..., weight_dtype="mxfp4_dense_only")):
//   out[M, N] = x[M, K] (bf16) . W_deq[N, K]^T,  W_deq = e2m1 code x 2^(scale byte - 127), one scale per row and 32 k
// on the codes and tile-major scales nvl_linear_wide_mxfp4 streams (nvl_quant_pack_mxfp4 + ops.tile_scales_mxfp4: no second
// layout, no second copy). It serves what that kernel's plan refuses — every M > 256 (prefill, decode batches of 257-512
// sequences) — so that the bf16 parameter the library GEMM needed can be released.
//
// Semantics. The weight enters the matrix instruction as bf16(code x scale) through v_cvt_scalef32_pk_bf16_fp4: exact under
// the EXACTNESS contract include/nvl.h states for nvl_linear_wide_mxfp4 (not widened here), so the result is x . W_deq^T with
// fp32 accumulation on v_mfma_f32_16x16x32_bf16, in this kernel's summation order.
//
// Decomposition. Above 256 rows the GEMM is bound by the matrix pipe and by what feeds it, not by the weight stream. A
// (16-row tile, 128-wide k step) is ONE KiB of codes but 16 packed converts per lane, so unlike gemm_tile_fp8.hip (2 x 2
// waves: the two waves of a column half convert the same bytes) every code is expanded ONCE per workgroup:
//   * workgroup = 4 consumer waves laid 1 x 4 + 1 loader wave. A consumer owns ALL BM rows of the workgroup and NT of its
//     4 NT column tiles; the x fragments are what the waves share, through LDS.
//   * tile shapes: 128 x 256 (MT = 8 row tiles, NT = 4: 128 fp32 accumulator registers per lane) or, while 4 x the
//     workgroups still fit the CUs in one round, 64 x 128 (MT = 4, NT = 2). The large shape is WIDE rather than
//     tall because 4-bit columns are the cheap operand: per 128-wide k step it reads 16 KiB of codes + 32 KiB of x for
//     128 x 256 outputs, where 256 x 128 would read 8 + 64 KiB and have every wave pull twice the x fragments out of LDS
//     per MFMA (a 1 x 4 wave reads the whole x stage).
//   * x operand: the loader wave stages x[BM, 64] (128 B per row: HALF a weight step) two half-steps ahead into three LDS
//     stages by LDS-DMA (global_load_lds_dwordx4, 8 rows per instruction); slot c of row r holds 16-byte chunk c ^ (r & 7),
//     so the 16 rows of a ds_read_b128 fragment read spread over all banks. One barrier per half-step. Three half-step
//     stages are 48 KiB at 128 rows — no LDS opt-in, so the entry is capturable from its first call; two or three full
//     128-column stages (64 / 96 KiB) would halve the barriers at twice the fragment registers per expansion group.
//     Rows past M read row M - 1 and are never stored.
//   * weight operand: global -> VGPR by the wave that owns the columns, RAW: 4 code dwords + 1 scale dword per (tile, step)
//     in a ring RING steps deep. A half-step expands its two k blocks (4 converts per fragment, the e8m0 byte shifted into
//     an fp32 exponent) once, shared by all MT row tiles; the slot is re-requested for step s + RING as soon as its second
//     half is expanded.
//   * per half-step a wave issues MT x NT x 2 MFMAs on NT independent chains; the x fragments of row tile mt + 1 are read
//     from LDS under the MFMAs of row tile mt.
//   * workgroup order: row blocks are the fast index inside bands of 8, so the workgroups in flight share a few weight
//     column groups AND a few x row blocks through L2.
//   * epilogue: bf16, 8-byte stores (a lane holds 4 consecutive columns of one row). SiLU: a wave's column tiles 2 j / 2 j + 1
//     are a gate tile and its up tile; the GEMM output is rounded to bf16 before the activation (nvl_linear_wide mode 1).
// Enqueue-only, no workspace: capturable. Row offsets are 64-bit (prefill m x k x 2 bytes passes 2^31).
#include "common.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>

namespace {

constexpr int kBK = 128;                 // k per weight step: one KiB of codes per column tile
constexpr int kHK = 64;                  // k per x half-step: two 32-wide MFMA k blocks
constexpr int kNS = 3;                   // x stages in LDS (the loader runs two half-steps ahead)
constexpr int kRowB = kHK * 2;           // bytes of one x row per half-step
constexpr int kNW = 4;                   // consumer waves (1 x 4)
constexpr int kTileStep = 1024;          // bytes of codes per (tile, step)
constexpr int kScaleStep = 64;           // bytes of scales per (tile, step)
enum { EPI_BF16 = 0, EPI_SILU = 1 };

__device__ __forceinline__ float silu_f32(float g) { return g / (1.f + __expf(-g)); }

// 8 codes (one dword: nibble j = element j) x 2^(byte - 127) -> the 8 bf16 of an MFMA A fragment
// (gemm_wide_mxfp4.hip::expand_fp4x8; operand byte `sel`, low nibble first)
__device__ __forceinline__ bf16x8_t expand_fp4x8(unsigned int c, unsigned int scale_byte) {
  const float scale = __uint_as_float(scale_byte << 23);
  u32x4_t r;
  r[0] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 0));
  r[1] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 1));
  r[2] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 2));
  r[3] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 3));
  return __builtin_bit_cast(bf16x8_t, r);
}

template <int MT, int NT, int RING>
__global__ __launch_bounds__((kNW + 1) * 64) void linear_tile_mxfp4_kernel(const bf16_t* __restrict__ x,
                                                                           const unsigned char* __restrict__ codes,
                                                                           const unsigned char* __restrict__ scales,
                                                                           bf16_t* __restrict__ out, int64_t M, int N, int K,
                                                                           int epi, int row_blocks, int col_groups) {
  constexpr int kRows = MT * 16;                                  // BM
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
  const int steps = K / kBK, last = steps - 1;                    // weight steps
  const int hsteps = 2 * steps, hlast = hsteps - 1;               // x half-steps

  if (wave >= kNW) {
    // ---- loader wave: x tile of half-step h + 2 -> LDS stage (h + 2) % 3 by LDS-DMA ----------------------------------------
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
    auto issue = [&](int h) {
      const unsigned dst = lds0 + (unsigned)(h % kNS) * kStage;
      const int koff = (h < hlast ? h : hlast) * kHK;
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
    // hsteps >= 2 = AHEAD always: a weight step is two half-steps
#pragma unroll
    for (int a = 0; a < AHEAD; ++a) issue(a);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kLC * (AHEAD - 1)) : "memory");     // half-step 0 has landed
    __builtin_amdgcn_s_barrier();
    for (int h = 0; h < hsteps; ++h) {
      // stage (h + AHEAD) % 3 was last read during half-step h - 1: free since the previous barrier
      if (h + AHEAD <= hlast) {
        issue(h + AHEAD);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kLC * (AHEAD - 1)) : "memory");  // half-steps up to h + 1 have landed
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
    }
    return;
  }

  // ---- consumer waves: wave w owns every row of the block x column tiles (kNW cgroup + w) NT ... ---------------------------
  const int ntiles = out_cols >> 4;                               // output column tiles (SiLU: gate / up pairs)
  const int unit0 = (cgroup * kNW + wave) * (silu ? NT / 2 : NT); // first output tile of this wave
  // wave-uniform bases of (tile nt, k step 0); the lane's share is one 32-bit offset
  const unsigned char* crow[NT];
  const unsigned char* srow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    int tile = unit0 + (silu ? nt >> 1 : nt);
    tile = tile < ntiles ? tile : ntiles - 1;                     // ragged last column group: any valid tile, masked at the store
    if (silu && (nt & 1)) tile += ntiles;                         // the up tile of that gate tile
    crow[nt] = codes + (int64_t)tile * steps * kTileStep;
    srow[nt] = scales + (int64_t)tile * steps * kScaleStep;
  }
  const int coff = lane * 16, soff = l15 * 4;
  int frag_off[2];                                                // B fragment of k block j of a half-step: row l15 of a row tile
#pragma unroll
  for (int j = 0; j < 2; ++j) frag_off[j] = l15 * kRowB + (((j * 4 + lq) ^ (l15 & 7)) << 4);

  f32x4_t acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  u32x4_t wf[RING][NT];                                           // raw codes, RING steps in flight
  unsigned int sc[RING][NT];                                      // their scale bytes (k blocks 0 .. 3 of the lane's row)
  auto wload = [&](u32x4_t* dst, unsigned int* sdst, int s) {
    const int64_t ks = s < last ? s : last;                       // prefetches past the end re-read the last step
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      dst[nt] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(crow[nt] + ks * kTileStep + coff));
      sdst[nt] = *reinterpret_cast<const unsigned int*>(srow[nt] + ks * kScaleStep + soff);
    }
  };

  // half H (k blocks 2 H, 2 H + 1) of one weight step on ring slot (wfs, scs) and LDS stage xs; LOAD: the slot is
  // re-requested for logical step sl as soon as its second half is expanded
  auto half = [&](auto half_tag, auto load_tag, const unsigned char* xs, u32x4_t* wfs, unsigned int* scs, int sl) {
    constexpr int H = decltype(half_tag)::value;
    constexpr bool LOAD = decltype(load_tag)::value;
    __builtin_amdgcn_sched_barrier(0);                             // (expansions stay inside their half-step)
    bf16x8_t a[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int j = 0; j < 2; ++j) a[nt][j] = expand_fp4x8(wfs[nt][2 * H + j], (scs[nt] >> (8 * (2 * H + j))) & 0xffu);
    if constexpr (LOAD && H == 1) wload(wfs, scs, sl);
    u32x4_t f[2][2];
    auto fread = [&](int mt, u32x4_t* dst) {
#pragma unroll
      for (int j = 0; j < 2; ++j) dst[j] = *reinterpret_cast<const u32x4_t*>(xs + mt * 16 * kRowB + frag_off[j]);
    };
    fread(0, f[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      if (mt + 1 < MT) fread(mt + 1, f[(mt + 1) & 1]);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)                            // NT independent chains, interleaved
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt][j], __builtin_bit_cast(bf16x8_t, f[mt & 1][j]),
                                                                acc[mt][nt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);                           // (keeps the reads of row tile mt + 2 out of this one)
    }
  };
  // one weight step s = two x half-steps 2 s, 2 s + 1 (stages (2 s) % 3, (2 s + 1) % 3), a barrier after each
  auto step = [&](auto load_tag, int s, u32x4_t* wfs, unsigned int* scs) {
    half(std::integral_constant<int, 0>{}, load_tag, smem + ((2 * s) % kNS) * kStage, wfs, scs, 0);
    __syncthreads();                                              // stage (h + 1) % 3 is staged, stage h % 3 is free
    half(std::integral_constant<int, 1>{}, load_tag, smem + ((2 * s + 1) % kNS) * kStage, wfs, scs, s + RING);
    __syncthreads();
  };

  // Pipeline invariant at the top of step s (slot i = s mod RING): LDS stage (2 s) % 3 holds x of half-step 2 s, slots
  // i .. i + RING - 1 hold (or have in flight) the codes and scales of steps s .. s + RING - 1.
#pragma unroll
  for (int r = 0; r < RING; ++r) wload(wf[r], sc[r], r);
  __syncthreads();                                                // stage 0 is staged
  const int nblk = steps / RING;
  for (int blk = 0; blk < nblk; ++blk) {
#pragma unroll
    for (int i = 0; i < RING; ++i) step(std::true_type{}, blk * RING + i, wf[i], sc[i]);
  }
#pragma unroll
  for (int i = 0; i < RING - 1; ++i) {
    const int s = nblk * RING + i;
    if (s < steps) step(std::false_type{}, s, wf[i], sc[i]);
  }

  // ---- epilogue: lane (l15, lq) holds out[row = 16 mt + l15][col = 16 tile + 4 lq .. + 3] ---------------------------------
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int64_t m = m_base + mt * 16 + l15;
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
// output column tiles (SiLU: gate / up pairs) of one workgroup
constexpr int units_per_wg(int nt, int epi) { return kNW * (epi == EPI_SILU ? nt / 2 : nt); }

template <int MT, int NT, int RING>
int launch_tile(const void* x, const void* codes, const void* scales, void* out, int64_t m, int n, int k, int epi, hipStream_t s) {
  constexpr size_t lds = (size_t)kNS * MT * 16 * kRowB;
  static_assert(lds <= 64 * 1024, "a larger stage set needs the hipFuncSetAttribute opt-in before the first capture");
  const int64_t row_blocks = (m + MT * 16 - 1) / (MT * 16);
  const int units = (epi == EPI_SILU ? n / 2 : n) / 16, per = units_per_wg(NT, epi);
  const int col_groups = (units + per - 1) / per;
  NVL_REQUIRE(row_blocks * col_groups < (1ll << 31), "nvl_linear_tile_mxfp4: m=%lld n=%d: grid too large", (long long)m, n);
  hipLaunchKernelGGL((linear_tile_mxfp4_kernel<MT, NT, RING>), dim3((unsigned)(row_blocks * col_groups)), dim3((kNW + 1) * 64),
                     lds, s, (const bf16_t*)x, (const unsigned char*)codes, (const unsigned char*)scales, (bf16_t*)out, m, n, k,
                     epi, (int)row_blocks, col_groups);
  return nvl_check_launch("nvl_linear_tile_mxfp4");
}

}  // namespace

extern "C" int nvl_linear_tile_mxfp4(const void* x, const void* codes, const void* scales_tiled, void* out, int64_t m, int n,
                                     int k, int mode, void* stream) {
  NVL_REQUIRE(x && codes && scales_tiled && out, "nvl_linear_tile_mxfp4: null pointer");
  NVL_REQUIRE(mode >= 0 && mode <= 2, "nvl_linear_tile_mxfp4: mode=%d (0 bf16, 1 silu*mul)", mode);
  NVL_REQUIRE(((uintptr_t)x | (uintptr_t)codes | (uintptr_t)scales_tiled | (uintptr_t)out) % 16 == 0,
              "nvl_linear_tile_mxfp4: pointers must be 16-byte aligned");
  // mode 2 (split-K fp32 partials) is not offered at these sizes: callers that want slabs take mode 0
  if (mode == 2 || m < 1 || k < kBK || k % kBK || n < 16 || n % (mode == EPI_SILU ? 32 : 16)) {
    nvl_set_error("nvl_linear_tile_mxfp4: shape m=%lld n=%d k=%d mode=%d not covered (m >= 1, k %% 128 == 0, n %% 16 == 0, "
                  "mode 1: n %% 32 == 0, modes 0 / 1)", (long long)m, n, k, mode);
    return NVL_EUNSUPPORTED;
  }
  // Tile shape: 64 x 128 only while ITS grid (4 x the workgroups) still fits the CUs in one round, else 128 x 256. Measured
  // (profiles/mxfp4_dense_only_tile.json, both shapes forced): a 64 x 128 workgroup runs at about half the rate per CU
  // (16 MFMAs per wave and barrier), so it wins at 64 large workgroups on 256 CUs (Qwen3-8B o / down at 512 rows: 34 vs
  // 51 us, 86 vs 132) and loses from 80 on (Qwen3-32B o at 512 rows: 104 vs 93 us; 160 workgroups: 107 vs 63).
  // NVL_TILE_MXFP4=big|small forces one (A/B measurements and the tests; the only switch of this kernel).
  const int units = (mode == EPI_SILU ? n / 2 : n) / 16, per = units_per_wg(4, mode);
  bool big = 4 * ((m + 127) / 128) * ((units + per - 1) / per) > nvl_device_cu_count();
  if (const char* e = getenv("NVL_TILE_MXFP4")) big = !strcmp(e, "big") ? true : !strcmp(e, "small") ? false : big;
  hipStream_t s = (hipStream_t)stream;
  return big ? launch_tile<8, 4, 2>(x, codes, scales_tiled, out, m, n, k, mode, s)
             : launch_tile<4, 2, 4>(x, codes, scales_tiled, out, m, n, k, mode, s);
}
