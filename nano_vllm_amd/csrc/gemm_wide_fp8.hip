// Weight-only FP8 (W8A16) wide-tile decode linear for gfx950:
//   out[M, N] = x[M, K] (bf16) . (W8[N, K] (OCP e4m3) o S)^T,  S fp32, one value per (16-row weight tile, 128-column k block)
// for decode steps (M <= 256) on the deep reductions of Qwen3-8B / 32B, full width and per rank. Same three outputs, output
// shapes, slab conventions and rounding points as nvl_linear_wide (gemm_wide.hip), so nvl_add_rmsnorm_splitk and the fused
// attention prologue consume its slabs unchanged.
//
// Semantics (what the tests hold it to). Per 128-column k block the products of x and the fp8 values (converted to bf16
// EXACTLY: every e4m3 value is a bf16 value) are accumulated in fp32 on the matrix pipe; that block sum is multiplied by the
// block's fp32 scale and added to the running fp32 accumulator. The scaled weight is never rounded to bf16, scales are
// arbitrary fp32.
//
// Why not gemm_wide.hip with a cast. That kernel's time is W bytes per CU / 18.6 GB/s + x bytes per CU / 67 GB/s (its
// header); halving W makes the x term as large as the W term, so the decomposition moves towards MORE COLUMNS PER WORKGROUP:
//   * workgroup = 3 consumer waves (one per SIMD, 512 registers each) + 1 loader wave. A consumer owns NT = 4 column tiles
//     (2 where N is too small for ~256 workgroups otherwise) x all row tiles of its row group: a raw fp8 fragment set costs
//     half the registers of a bf16 one, so the ring holds twice the tiles for the same bytes in flight, the workgroup covers
//     192 columns and the x bytes per CU halve. Where that leaves too few workgroups the plan refills with a K split
//     (fp32 slabs, as the bf16 kernel).
//   * packed weights [N/16 tiles][K/64][64 lanes][16 bytes] (nvl_pack_weight_tiles_fp8): a lane's 16 bytes are its A
//     fragments of two consecutive 32-wide k blocks of v_mfma_f32_16x16x32_bf16 (bytes 0-7: k = 64 j + 8 lq ..., bytes 8-15:
//     k = 64 j + 32 + 8 lq ...; lane = 16 lq + row % 16). One wave load = one contiguous KiB, non-temporal, two MFMAs per row
//     tile after conversion; a 128-column step is two such loads per tile.
//   * the ring holds RAW fp8 (RING steps in flight: a slot is converted to bf16 at the top of its step with
//     v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 — 8 packed conversions per 16-byte load — and re-requested at once for step
//     s + RING). The tile's scale of that step travels in the same slot (one broadcast dword load per tile and step, in
//     order with the weight loads: a wave reads its tile's scale row exactly once).
//   * scale application without a second accumulator set: inside a step the row tiles are the OUTER loop and the four k
//     blocks the inner one; the block sums of one row tile x NT column tiles live in NT x 4 registers (NT independent MFMA
//     chains, interleaved), and are folded into the running accumulators with one fma per value.
//   * x staging is gemm_wide.hip's loader: LDS-DMA of the [rows, 128] tile two steps ahead into three XOR-swizzled stages,
//     one barrier per step, a rotated K walk per workgroup; straight-line RING-step loop body with unconditional
//     (index-clamped) loads so hipcc's s_waitcnt stays counted.
//   * 145-256 rows: two row groups (<= 9 row tiles each) whose workgroups are dispatched back to back on the same XCD
//     (`paired_tiles`, as gemm_wide.hip): the partner's weight lines hit that XCD's L2.
#include "common.h"
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr int kBK = 128;                 // k per step = one scale block
constexpr int kKB = kBK / 32;            // 32-wide MFMA k blocks per step
constexpr int kNW = 3;                   // consumer waves per workgroup
constexpr int kNS = 3;                   // x stages in LDS (the loader runs two steps ahead)
constexpr int kRowB = kBK * 2;           // bytes of one x row per step
enum { EPI_BF16 = 0, EPI_SILU = 1, EPI_PARTIAL = 2 };

__device__ __forceinline__ float silu_f32(float g) { return g / (1.f + __expf(-g)); }

// 8 fp8 (two dwords) -> 8 bf16 in MFMA operand order (element e = byte e), exact
__device__ __forceinline__ bf16x8_t fp8x8_to_bf16x8(unsigned lo, unsigned hi) {
  u32x4_t r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
  return __builtin_bit_cast(bf16x8_t, r);
}

// `epi` is a launch argument, not a template parameter (the three outputs differ in the tile mapping and the stores only).
// SiLU: a wave's tiles 2 j / 2 j + 1 are a gate tile and its up tile.
template <int MT, int NT, int RING>
__global__ __launch_bounds__((kNW + 1) * 64) void linear_wide_fp8_kernel(const bf16_t* __restrict__ x,
                                                                         const unsigned char* __restrict__ w8,
                                                                         const float* __restrict__ scales,
                                                                         void* __restrict__ out, int M, int N, int K,
                                                                         int steps, int epi, int paired_tiles) {
  constexpr int kRows = MT * 16;
  constexpr int kStage = kRows * kRowB;                           // bytes per LDS stage
  constexpr int AHEAD = kNS - 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  // (tile, row group): plain (blockIdx.x, blockIdx.z); two row groups are folded into blockIdx.x so that the two
  // partners of a column tile run on the same XCD (ids 16 g + c and 16 g + 8 + c), see gemm_wide.hip
  int tile_x = blockIdx.x, rgroup = blockIdx.z;
  if (paired_tiles > 0) {
    tile_x = (int)(blockIdx.x >> 4) * 8 + (int)(blockIdx.x & 7);
    rgroup = (int)(blockIdx.x >> 3) & 1;
    if (tile_x >= paired_tiles) return;                           // grid padding (whole workgroup, before any barrier)
  }
  const int m_base = rgroup * kRows;
  const bool silu = epi == EPI_SILU;
  const int out_cols = silu ? N / 2 : N;
  const int ksteps = K / kBK;
  const int64_t s0 = (int64_t)blockIdx.y * steps;                 // first k step of this workgroup's K range
  const int last = steps - 1;
  // rotated K walk: lock-step walkers would all hit the same offset of the tiles' K-byte stride at once
  const int rot = (int)(((unsigned)tile_x + 3u * blockIdx.y) % (unsigned)steps);
  auto kstep = [&](int s) {                                       // logical step (prefetches past the end clamp) -> k step
    s = (s < last ? s : last) + rot;
    return s >= steps ? s - steps : s;
  };

  if (wave >= kNW) {
    // ---- loader wave: x tile of step s + 2 -> LDS stage (s + 2) % 3 by LDS-DMA (gemm_wide.hip's scheme) ---------------
    // instruction i covers rows 4 i + lq, 16-byte slots l15; slot l15 of row r holds chunk l15 ^ (r & 15)
    constexpr int kLC = kRows / 4;                                // 1-KiB pieces of a tile
    static_assert(kLC * (AHEAD - 1) < 64, "vmcnt is a 6-bit counter");
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const bf16_t* xb = x + s0 * kBK;
    int x_src[kLC];                                               // element offsets (M * K < 2^31)
#pragma unroll
    for (int i = 0; i < kLC; ++i) {
      const int row = 4 * i + lq;
      int grow = m_base + row;
      grow = grow < M ? grow : M - 1;                             // padding rows read a valid row (never stored)
      x_src[i] = grow * K + ((l15 ^ (row & 15)) << 3);
    }
    auto issue = [&](int s) {
      const unsigned dst = lds0 + (unsigned)(s % kNS) * kStage;
      const bf16_t* src = xb + kstep(s) * kBK;
#pragma unroll
      for (int i = 0; i < kLC; ++i) {
        unsigned keep;
        const unsigned d = __builtin_amdgcn_readfirstlane(dst + i * 1024);
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(src + x_src[i]), "s"(d)
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

  // ---- consumer waves --------------------------------------------------------------------------------------------------
  const int ntiles = out_cols >> 4;                               // output column tiles (SiLU: gate / up pairs)
  const int unit0 = (tile_x * kNW + wave) * (silu ? NT / 2 : NT); // first output tile of this wave
  const unsigned char* wrow[NT];                                  // lane's 16 bytes of (tile nt, first k step of the range)
  const float* srow[NT];                                          // scale row of tile nt at the range's first k block
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    int tile = unit0 + (silu ? nt >> 1 : nt);
    tile = tile < ntiles ? tile : ntiles - 1;                     // ragged last workgroup: any valid tile, masked at the store
    if (silu && (nt & 1)) tile += ntiles;                         // the up tile of that gate tile
    wrow[nt] = w8 + (int64_t)tile * 16 * K + s0 * 2048 + lane * 16;
    srow[nt] = scales + (int64_t)tile * ksteps + s0;
  }
  int frag_off[kKB];                                              // B fragment of k block kb: row l15 of a row tile
#pragma unroll
  for (int kb = 0; kb < kKB; ++kb) frag_off[kb] = l15 * 256 + (((kb * 4 + lq) ^ l15) << 4);

  f32x4_t acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  u32x4_t wf[RING][NT][2];                                        // raw fp8 fragments, RING steps in flight
  float sc[RING][NT];
  auto wload = [&](u32x4_t (*dst)[2], float* sdst, int s) {
    const int ks = kstep(s);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
        dst[nt][h] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wrow[nt] + ks * 2048 + h * 1024));
      sdst[nt] = srow[nt][ks];
    }
  };

  // one k step on ring slot (wfs, scs) and LDS stage xs; LOAD: the slot is re-requested for logical step sl as soon as
  // its fragments are converted
  auto compute = [&](auto load_tag, const unsigned char* xs, u32x4_t (*wfs)[2], float* scs, int sl) {
    constexpr bool LOAD = decltype(load_tag)::value;
    __builtin_amdgcn_sched_barrier(0);                             // (conversions stay inside their step)
    bf16x8_t a[NT][kKB];
    float s[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        a[nt][2 * h] = fp8x8_to_bf16x8(wfs[nt][h][0], wfs[nt][h][1]);
        a[nt][2 * h + 1] = fp8x8_to_bf16x8(wfs[nt][h][2], wfs[nt][h][3]);
      }
      s[nt] = scs[nt];
    }
    if constexpr (LOAD) wload(wfs, scs, sl);
    // the x fragments of row tile mt + 1 are read under the MFMAs of row tile mt; the scheduling barriers keep hipcc from
    // hoisting every row tile's reads (MT x 16 registers) to the top of the step
    u32x4_t f[2][kKB];
    auto fread = [&](int mt, u32x4_t* dst) {
#pragma unroll
      for (int kb = 0; kb < kKB; ++kb) dst[kb] = *reinterpret_cast<const u32x4_t*>(xs + mt * 16 * kRowB + frag_off[kb]);
    };
    fread(0, f[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      if (mt + 1 < MT) fread(mt + 1, f[(mt + 1) & 1]);
      f32x4_t bs[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bs[nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < kKB; ++kb)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)                            // NT independent chains, interleaved
          bs[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt][kb], __builtin_bit_cast(bf16x8_t, f[mt & 1][kb]), bs[nt], 0, 0, 0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mt][nt][r] = __builtin_fmaf(bs[nt][r], s[nt], acc[mt][nt][r]);
      // (pins the fold HERE: hipcc otherwise sinks the fmas of all RING steps to the end of the loop body and keeps every
      //  block sum alive until then — 16 registers per row tile and step)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) asm volatile("" : "+v"(acc[mt][nt]));
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // Pipeline invariant at the top of step s (slot i = s mod RING): LDS stage s % 3 holds x of step s, slots i .. i + RING - 1
  // hold (or have in flight) the weights and scales of steps s .. s + RING - 1.
#pragma unroll
  for (int r = 0; r < RING; ++r) wload(wf[r], sc[r], r);
  __syncthreads();                                                // stage 0 is staged
  const int nblk = steps / RING;
  for (int blk = 0; blk < nblk; ++blk) {
#pragma unroll
    for (int i = 0; i < RING; ++i) {
      const int s = blk * RING + i;
      compute(std::true_type{}, smem + (s % kNS) * kStage, wf[i], sc[i], s + RING);
      __syncthreads();                                            // stage (s + 1) % 3 is staged, stage s % 3 is free
    }
  }
#pragma unroll
  for (int i = 0; i < RING - 1; ++i) {
    const int s = nblk * RING + i;
    if (s < steps) {
      compute(std::false_type{}, smem + (s % kNS) * kStage, wf[i], sc[i], 0);
      __syncthreads();
    }
  }

  // ---- epilogue: lane (l15, lq) holds out[row = 16 mt + l15][col = 16 tile + 4 lq .. + 3] ---------------------------------
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m_base + mt * 16 + l15;
    if (m >= M) continue;
    if (silu) {
#pragma unroll
      for (int j = 0; j < NT / 2; ++j) {
        if (unit0 + j >= ntiles) continue;
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = silu_f32(round_bf16(acc[mt][2 * j][r])) * round_bf16(acc[mt][2 * j + 1][r]);
        u32x2_t ov = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
        *reinterpret_cast<u32x2_t*>((bf16_t*)out + (int64_t)m * out_cols + (unit0 + j) * 16 + lq * 4) = ov;
      }
    } else {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if (unit0 + nt >= ntiles) continue;
        const int n = (unit0 + nt) * 16 + lq * 4;
        if (epi == EPI_BF16) {
          u32x2_t o = {pack_bf16x2(acc[mt][nt][0], acc[mt][nt][1]), pack_bf16x2(acc[mt][nt][2], acc[mt][nt][3])};
          *reinterpret_cast<u32x2_t*>((bf16_t*)out + (int64_t)m * N + n) = o;
        } else {
          *reinterpret_cast<f32x4_t*>((float*)out + ((int64_t)blockIdx.y * M + m) * N + n) = acc[mt][nt];
        }
      }
    }
  }
}

// out = epilogue(sum_s part[s]) for bf16 / SiLU outputs whose GEMM was split over K (gemm_wide.hip's reduce: 4 output
// columns per thread, slabs summed in split order, the sum rounded to bf16 before the activation)
template <int EPI>
__global__ __launch_bounds__(256) void slab_reduce_fp8_kernel(const float* __restrict__ part, int splits, int64_t split_stride,
                                                               bf16_t* __restrict__ out, int M, int N) {
  const int out_cols = EPI == EPI_SILU ? N / 2 : N;
  const int qpr = out_cols >> 2;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (int64_t)M * qpr) return;
  const int row = (int)(q / qpr), c = (int)(q - (int64_t)row * qpr) * 4;
  const float* p = part + (int64_t)row * N + c;
  f32x4_t a = *reinterpret_cast<const f32x4_t*>(p);
  f32x4_t b = {0.f, 0.f, 0.f, 0.f};
  if constexpr (EPI == EPI_SILU) b = *reinterpret_cast<const f32x4_t*>(p + out_cols);
  for (int s = 1; s < splits; ++s) {
    a += *reinterpret_cast<const f32x4_t*>(p + s * split_stride);
    if constexpr (EPI == EPI_SILU) b += *reinterpret_cast<const f32x4_t*>(p + s * split_stride + out_cols);
  }
  float o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = EPI == EPI_SILU ? silu_f32(round_bf16(a[r])) * round_bf16(b[r]) : a[r];
  u32x2_t ov = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
  *reinterpret_cast<u32x2_t*>(out + (int64_t)row * out_cols + c) = ov;
}

// W8 [N, K] row-major e4m3 -> packed [N/16][K/64][64 lanes][16 bytes]: thread = one 16-byte chunk of the destination
__global__ __launch_bounds__(256) void pack_weight_tiles_fp8_kernel(const unsigned char* __restrict__ w,
                                                                     unsigned char* __restrict__ packed, int64_t chunks, int K) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= chunks) return;
  const int lane = (int)(c & 63);
  const int64_t blk = c >> 6;                                     // (tile, 64-column k chunk)
  const int kchunks = K >> 6;
  const int64_t tile = blk / kchunks;
  const int kc = (int)(blk - tile * kchunks);
  const unsigned char* src = w + (tile * 16 + (lane & 15)) * K + kc * 64 + (lane >> 4) * 8;
  const u32x2_t lo = *reinterpret_cast<const u32x2_t*>(src), hi = *reinterpret_cast<const u32x2_t*>(src + 32);
  *reinterpret_cast<u32x4_t*>(packed + c * 16) = u32x4_t{lo[0], lo[1], hi[0], hi[1]};
}

// ---- host: plan ------------------------------------------------------------------------------------------------------
struct Fp8Plan { int mt, nt, mgroups, tiles, split, steps; };

// Ring depth: 32 KiB (NT = 4) / 24 KiB (NT = 2) of raw fragments in flight per wave; NT = 4 with <= 3 row tiles takes one
// step less (hipcc's allocation of the 4-deep form spills 2-3 registers there, tests/test_kernel_resources.py)
constexpr int ring_of(int nt, int mt) { return nt == 4 ? (mt <= 3 ? 3 : 4) : 6; }

int round_mt(int mtiles) {
  static const int kMT[] = {1, 2, 3, 5, 7, 9};
  for (int c : kMT)
    if (c >= mtiles) return c;
  return 0;
}

// Columns per wave (NT) and K split, deterministically from the shape. Model of a launch (us): rounds of 256 workgroups x
// steps x (W bytes of a step / 18.6 GB/s + x bytes of a step / 67 GB/s: the two measured per-CU rates of gemm_wide.hip's
// time model, which ADD) + the pipeline fill per round + the slab traffic of a split (gemm_wide.hip::wide_cost's terms).
// PREDICTED rates for this kernel, not fitted ones: tools/gemm_fp8_bench.py records what the plans measure.
bool fp8_plan(int64_t m, int n, int k, int mode, Fp8Plan* best) {
  if (m < 1 || m > 256 || n < 16 || k < kBK || k % kBK) return false;
  if (m * (int64_t)k >= (1ll << 31)) return false;                // 32-bit x element offsets in the loader
  if (mode == EPI_SILU ? n % 32 : n % 16) return false;
  const int mtiles = (int)((m + 15) / 16), ksteps = k / kBK;
  Fp8Plan p;
  p.mgroups = mtiles > 9 ? 2 : 1;
  p.mt = round_mt((mtiles + p.mgroups - 1) / p.mgroups);
  const int max_split = mode == EPI_PARTIAL ? 8 : 16;             // (consumers of the slabs take at most 8)
  double best_t = 1e30;
  for (int nt : {4, 2}) {
    p.nt = nt;
    const double t_step = kNW * nt * 2048.0 / 18.6e3 + p.mt * 16 * 256.0 / 67.0e3;
    for (int split = 1; split <= max_split; ++split) {
      if (ksteps % split || (split > 1 && ksteps / split < 2)) continue;
      p.split = split;
      p.steps = ksteps / split;
      // a split bf16 / SiLU launch tiles all n columns (the reduce kernel forms the SiLU pairs)
      const int cols = kNW * nt * 16, units = mode == EPI_SILU && split == 1 ? n / 2 : n;
      p.tiles = (units + (mode == EPI_SILU && split == 1 ? cols / 2 : cols) - 1) / (mode == EPI_SILU && split == 1 ? cols / 2 : cols);
      const int wgs = p.tiles * split * p.mgroups;
      double t = (double)((wgs + 255) / 256) * (p.steps * t_step + 2.0) + 2.5;
      if (split > 1 || mode == EPI_PARTIAL) {
        const double slab = (double)split * m * n * 4.0;
        t += slab / 4.0e6;
        if (mode != EPI_PARTIAL) t += slab / 4.0e6 + 3.5;
        else t += (split - 1) * (double)m * n * 4.0 / 6.0e6;
      }
      if (t < best_t) { best_t = t; *best = p; }
    }
  }
  return best_t < 1e30;
}

template <int MT, int NT>
int launch_fp8(const Fp8Plan& p, const void* x, const void* w8, const void* scales, void* out, int64_t m, int n, int k, int epi,
               hipStream_t s) {
  constexpr int RING = ring_of(NT, MT);
  const size_t lds = (size_t)kNS * MT * 16 * kRowB;
  static bool attr_done[NVL_MAX_DEVICES] = {};
  bool& attr_set = attr_done[nvl_device_slot()];
  if (!attr_set && lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&linear_wide_fp8_kernel<MT, NT, RING>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      nvl_set_error("nvl_linear_wide_fp8: cannot reserve %zu B of LDS", lds);
      return NVL_ELAUNCH;
    }
    attr_set = true;
  }
  const dim3 grid = p.mgroups == 2 ? dim3((unsigned)((p.tiles + 7) / 8) * 16, p.split, 1) : dim3(p.tiles, p.split, 1);
  hipLaunchKernelGGL((linear_wide_fp8_kernel<MT, NT, RING>), grid, dim3((kNW + 1) * 64), lds, s, (const bf16_t*)x,
                     (const unsigned char*)w8, (const float*)scales, out, (int)m, n, k, p.steps, epi,
                     p.mgroups == 2 ? p.tiles : 0);
  return NVL_OK;
}

int dispatch_fp8(const Fp8Plan& p, const void* x, const void* w8, const void* scales, void* out, int64_t m, int n, int k, int epi,
                 hipStream_t s) {
#define NVL_F8(MT_) \
  if (p.mt == MT_) return p.nt == 4 ? launch_fp8<MT_, 4>(p, x, w8, scales, out, m, n, k, epi, s) \
                                    : launch_fp8<MT_, 2>(p, x, w8, scales, out, m, n, k, epi, s);
  NVL_F8(1) NVL_F8(2) NVL_F8(3) NVL_F8(5) NVL_F8(7) NVL_F8(9)
#undef NVL_F8
  nvl_set_error("nvl_linear_wide_fp8: internal plan error (mt=%d nt=%d)", p.mt, p.nt);
  return NVL_EINVAL;
}

}  // namespace

extern "C" int nvl_linear_wide_fp8_plan(int64_t m, int n, int k, int mode, int* splits, size_t* workspace_bytes) {
  Fp8Plan p;
  if (mode < 0 || mode > 2 || !fp8_plan(m, n, k, mode, &p)) return 0;
  if (splits) *splits = p.split;
  if (workspace_bytes) *workspace_bytes = mode != EPI_PARTIAL && p.split > 1 ? (size_t)p.split * m * n * sizeof(float) : 0;
  return 1;
}

extern "C" int nvl_pack_weight_tiles_fp8(const void* weight, void* packed, int64_t n, int64_t k, void* stream) {
  NVL_REQUIRE(weight && packed && weight != packed, "nvl_pack_weight_tiles_fp8: null or aliased pointers");
  NVL_REQUIRE(n > 0 && k > 0 && n % 16 == 0 && k % 64 == 0 && k < (1ll << 31),
              "nvl_pack_weight_tiles_fp8: n=%lld must be a multiple of 16, k=%lld of 64", (long long)n, (long long)k);
  NVL_REQUIRE(((uintptr_t)weight | (uintptr_t)packed) % 16 == 0, "nvl_pack_weight_tiles_fp8: pointers must be 16-byte aligned");
  const int64_t chunks = n * k / 16;
  NVL_REQUIRE((chunks + 255) / 256 < (1ll << 31), "nvl_pack_weight_tiles_fp8: matrix too large");
  hipLaunchKernelGGL(pack_weight_tiles_fp8_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)weight, (unsigned char*)packed, chunks, (int)k);
  return nvl_check_launch("nvl_pack_weight_tiles_fp8");
}

extern "C" int nvl_linear_wide_fp8(const void* x, const void* w8_packed, const void* scales, void* out, int64_t m, int n, int k,
                                   int mode, void* workspace, size_t workspace_bytes, void* stream) {
  NVL_REQUIRE(x && w8_packed && scales && out, "nvl_linear_wide_fp8: null pointer");
  NVL_REQUIRE(mode >= 0 && mode <= 2, "nvl_linear_wide_fp8: mode=%d (0 bf16, 1 silu*mul, 2 split-K fp32 partials)", mode);
  NVL_REQUIRE(((uintptr_t)x | (uintptr_t)w8_packed | (uintptr_t)out | (uintptr_t)workspace) % 16 == 0 && (uintptr_t)scales % 4 == 0,
              "nvl_linear_wide_fp8: pointers must be 16-byte aligned (scales: 4)");
  Fp8Plan p;
  if (!fp8_plan(m, n, k, mode, &p)) {
    nvl_set_error("nvl_linear_wide_fp8: shape m=%lld n=%d k=%d mode=%d not covered (query nvl_linear_wide_fp8_plan first)",
                  (long long)m, n, k, mode);
    return NVL_EUNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  if (mode == EPI_PARTIAL || p.split == 1) {
    const int rc = dispatch_fp8(p, x, w8_packed, scales, out, m, n, k, mode, s);
    return rc != NVL_OK ? rc : nvl_check_launch("nvl_linear_wide_fp8");
  }
  const size_t need = (size_t)p.split * m * n * sizeof(float);
  NVL_REQUIRE(workspace && workspace_bytes >= need, "nvl_linear_wide_fp8: workspace %zu B < required %zu B", workspace_bytes, need);
  const int rc = dispatch_fp8(p, x, w8_packed, scales, workspace, m, n, k, EPI_PARTIAL, s);
  if (rc != NVL_OK) return rc;
  const int out_cols = mode == EPI_SILU ? n / 2 : n;
  const unsigned blocks = (unsigned)((m * (int64_t)(out_cols / 4) + 255) / 256);
  if (mode == EPI_SILU)
    hipLaunchKernelGGL(slab_reduce_fp8_kernel<EPI_SILU>, dim3(blocks), dim3(256), 0, s, (const float*)workspace, p.split,
                       (int64_t)m * n, (bf16_t*)out, (int)m, n);
  else
    hipLaunchKernelGGL(slab_reduce_fp8_kernel<EPI_BF16>, dim3(blocks), dim3(256), 0, s, (const float*)workspace, p.split,
                       (int64_t)m * n, (bf16_t*)out, (int)m, n);
  return nvl_check_launch("nvl_linear_wide_fp8");
}
