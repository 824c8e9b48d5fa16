// Weight-only MXFP4 (W4A16) wide-tile decode linear for gfx950 (LLM(..., weight_dtype="mxfp4_dense")):
//   out[M, N] = x[M, K] (bf16) . W_deq[N, K]^T,  W_deq = e2m1 code x 2^(scale byte - 127), one scale per row and 32 k
// for decode steps (M <= 256) on the deep reductions of Qwen3-8B / 32B. Same three outputs, output shapes, slab
// conventions and rounding points as nvl_linear_wide (gemm_wide.hip), so nvl_add_rmsnorm_splitk and the fused attention
// prologue consume its slabs unchanged. The format and the quantiser are moe_mxfp4.hip's (nvl_quant_pack_mxfp4).
//
// Semantics. code x scale is a bf16 value (one significant bit of mantissa, a power-of-two scale), so the matrix
// instruction receives bf16(W_deq) EXACTLY wherever the product is a normal bf16, and the kernel computes x . W_deq^T
// with fp32 accumulation on v_mfma_f32_16x16x32_bf16 — nothing else is rounded. The scale therefore goes in at the
// conversion: no per-block second accumulator, no fma fold (the bs[] stage of gemm_wide_fp8.hip and its registers).
//
// Decomposition. A (16-row tile, 128-wide k step) of codes is ONE KiB (bf16: 4, fp8: 2), so in the project's time model
// (W bytes per CU / 18.6 GB/s + x bytes per CU / 67 GB/s, gemm_wide.hip) the x term dominates, and the workgroup goes
// wider than the fp8 kernel's:
//   * workgroup = 3 consumer waves (one per SIMD, 512 registers each) + 1 loader wave. A consumer owns NT = 8 / 4 / 2
//     column tiles x all row tiles of its row group: up to 384 columns per workgroup, 288 accumulator registers at 9 row
//     tiles. Where that leaves too few workgroups the plan refills the grid with a K split (fp32 slabs).
//   * codes [N/16][K/128][64 lanes][16 bytes], exactly what nvl_quant_pack_mxfp4 writes: a lane's 16 bytes are its four A
//     fragments of the step (dword kb = 8 codes of k block kb, k = 32 kb + 8 lq ...). One non-temporal wave load = one
//     contiguous KiB.
//   * scales in a TILE-MAJOR layout of their own, uint8 [N/16][K/128][16 rows][4 k blocks]: a tile step's scales are one
//     contiguous 64-byte line, lane (l15, .) reads its row's four as one dword. (The quantiser's row-major [N][K/32]
//     would scatter a tile step over 16 lines.) The re-layout is made once at load (ops.tile_scales_mxfp4).
//   * the ring holds RAW steps: 4 code registers + 1 scale dword per tile step, RING steps in flight. A slot is expanded
//     in registers with v_cvt_scalef32_pk_bf16_fp4 — four per fragment, the e8m0 byte shifted into an fp32 exponent —
//     and re-requested for step s + RING as soon as its last fragment is converted. NT <= 4 expands the whole step at its
//     top; NT = 8 one k block at a time (the expanded fragments of 8 tiles x 4 blocks would be 128 registers).
//     NT = 8 stops at 7 row tiles: at 9 (288 accumulators) hipcc's allocation of the unrolled ring — it copies the
//     slots between names at the loop head — spills even two steps deep, and no instantiation may spill.
//   * x staging is gemm_wide.hip's loader, re-stated here: LDS-DMA (global_load_lds_dwordx4) of the [rows, 128] tile two
//     steps ahead into three XOR-swizzled stages, one barrier per step, a rotated K walk per workgroup, a straight-line
//     RING-step loop body with unconditional (index-clamped) loads so hipcc's s_waitcnt stays counted.
//   * 145-256 rows: two row groups (<= 9 row tiles each) whose workgroups are dispatched back to back on the same XCD
//     (`paired_tiles`, as gemm_wide.hip): the partner's code lines hit that XCD's L2.
//   * the ragged last workgroup clamps to a valid tile and masks at the store; padding rows read a valid row and are
//     never stored.
#include "common.h"
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr int kBK = 128;                 // k per step
constexpr int kKB = kBK / 32;            // 32-wide MFMA k blocks (= scale blocks) per step
constexpr int kNW = 3;                   // consumer waves per workgroup
constexpr int kNS = 3;                   // x stages in LDS (the loader runs two steps ahead)
constexpr int kRowB = kBK * 2;           // bytes of one x row per step
constexpr int kTileStep = 1024;          // bytes of codes per (tile, step)
constexpr int kScaleStep = 64;           // bytes of scales per (tile, step)
enum { EPI_BF16 = 0, EPI_SILU = 1, EPI_PARTIAL = 2 };

__device__ __forceinline__ float silu_f32(float g) { return g / (1.f + __expf(-g)); }

// 8 codes (one dword: nibble j = element j) x 2^(byte - 127) -> the 8 bf16 of an MFMA A fragment
// (moe_mxfp4.hip::expand_fp4x8; operand byte `sel`, low nibble first)
__device__ __forceinline__ bf16x8_t expand_fp4x8(unsigned int c, unsigned int scale_byte) {
  const float scale = __uint_as_float(scale_byte << 23);
  u32x4_t r;
  r[0] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 0));
  r[1] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 1));
  r[2] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 2));
  r[3] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 3));
  return __builtin_bit_cast(bf16x8_t, r);
}

// `epi` is a launch argument, not a template parameter (the three outputs differ in the tile mapping and the stores only).
// SiLU: a wave's tiles 2 j / 2 j + 1 are a gate tile and its up tile.
template <int MT, int NT, int RING>
__global__ __launch_bounds__((kNW + 1) * 64) void linear_wide_mxfp4_kernel(const bf16_t* __restrict__ x,
                                                                           const unsigned char* __restrict__ codes,
                                                                           const unsigned char* __restrict__ scales,
                                                                           void* __restrict__ out, int M, int N, int K,
                                                                           int steps, int epi, int paired_tiles) {
  constexpr int kRows = MT * 16;
  constexpr int kStage = kRows * kRowB;                           // bytes per LDS stage
  constexpr int AHEAD = kNS - 1;
  constexpr int KG = NT == 8 ? 1 : kKB;                           // k blocks expanded at a time
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
  // rotated K walk: lock-step walkers would all hit the same offset of the tiles' stride at once
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
  // wave-uniform bases of (tile nt, first k step of the range); the lane's share is one 32-bit offset
  const unsigned char* crow[NT];
  const unsigned char* srow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    int tile = unit0 + (silu ? nt >> 1 : nt);
    tile = tile < ntiles ? tile : ntiles - 1;                     // ragged last workgroup: any valid tile, masked at the store
    if (silu && (nt & 1)) tile += ntiles;                         // the up tile of that gate tile
    const int64_t ts = (int64_t)tile * ksteps + s0;
    crow[nt] = codes + ts * kTileStep;
    srow[nt] = scales + ts * kScaleStep;
  }
  const int coff = lane * 16, soff = l15 * 4;
  int frag_off[kKB];                                              // B fragment of k block kb: row l15 of a row tile
#pragma unroll
  for (int kb = 0; kb < kKB; ++kb) frag_off[kb] = l15 * 256 + (((kb * 4 + lq) ^ l15) << 4);

  f32x4_t acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  u32x4_t wf[RING][NT];                                           // raw codes, RING steps in flight
  unsigned int sc[RING][NT];                                      // their scale bytes (k blocks 0 .. 3 of the lane's row)
  auto wload = [&](u32x4_t* dst, unsigned int* sdst, int s) {
    const int ks = kstep(s);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      dst[nt] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(crow[nt] + ks * kTileStep + coff));
      sdst[nt] = *reinterpret_cast<const unsigned int*>(srow[nt] + ks * kScaleStep + soff);
    }
  };

  // one k step on ring slot (wfs, scs) and LDS stage xs; LOAD: the slot is re-requested for logical step sl as soon as
  // its last fragment is expanded
  auto compute = [&](auto load_tag, const unsigned char* xs, u32x4_t* wfs, unsigned int* scs, int sl) {
    constexpr bool LOAD = decltype(load_tag)::value;
#pragma unroll
    for (int g = 0; g < kKB; g += KG) {
      __builtin_amdgcn_sched_barrier(0);                           // (expansions stay inside their step)
      bf16x8_t a[NT][KG];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < KG; ++j) a[nt][j] = expand_fp4x8(wfs[nt][g + j], (scs[nt] >> (8 * (g + j))) & 0xffu);
      if constexpr (LOAD)
        if (g + KG == kKB) wload(wfs, scs, sl);
      // the x fragments of row tile mt + 1 are read under the MFMAs of row tile mt; the scheduling barriers keep hipcc
      // from hoisting every row tile's reads (MT x 4 KG registers) to the top of the step
      u32x4_t f[2][KG];
      auto fread = [&](int mt, u32x4_t* dst) {
#pragma unroll
        for (int j = 0; j < KG; ++j) dst[j] = *reinterpret_cast<const u32x4_t*>(xs + mt * 16 * kRowB + frag_off[g + j]);
      };
      fread(0, f[0]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (mt + 1 < MT) fread(mt + 1, f[(mt + 1) & 1]);
#pragma unroll
        for (int j = 0; j < KG; ++j)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)                          // NT independent chains, interleaved
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt][j], __builtin_bit_cast(bf16x8_t, f[mt & 1][j]),
                                                                  acc[mt][nt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  // Pipeline invariant at the top of step s (slot i = s mod RING): LDS stage s % 3 holds x of step s, slots i .. i + RING - 1
  // hold (or have in flight) the codes and scales of steps s .. s + RING - 1.
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
__global__ __launch_bounds__(256) void slab_reduce_mxfp4_kernel(const float* __restrict__ part, int splits,
                                                                 int64_t split_stride, bf16_t* __restrict__ out, int M, int N) {
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

// codes [N/16][K/128][64][16] + row-major scales [N][K/32] -> W_deq [N, K] bf16 row-major: thread = one lane's 16 bytes of
// a (tile, step) — its four fragments, 8 consecutive k each — expanded by the same instruction as the GEMM's
__global__ __launch_bounds__(256) void unpack_mxfp4_kernel(const unsigned char* __restrict__ codes,
                                                           const unsigned char* __restrict__ scales,
                                                           bf16_t* __restrict__ w, int64_t chunks, int ksteps, int64_t K) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= chunks) return;
  const int lane = (int)(c & 63), l15 = lane & 15, lq = lane >> 4;
  const int64_t item = c >> 6, tile = item / ksteps;
  const int s = (int)(item - tile * ksteps);
  const int64_t row = tile * 16 + l15;
  const u32x4_t cw = *reinterpret_cast<const u32x4_t*>(codes + c * 16);
  const unsigned int sb = *reinterpret_cast<const unsigned int*>(scales + row * (K >> 5) + s * 4);
  bf16_t* dst = w + row * K + s * 128 + lq * 8;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
    *reinterpret_cast<bf16x8_t*>(dst + kb * 32) = expand_fp4x8(cw[kb], (sb >> (8 * kb)) & 0xffu);
}

// ---- host: plan ------------------------------------------------------------------------------------------------------
struct Fp4Plan { int mt, nt, mgroups, tiles, split, steps; };

// Ring depth (raw steps in flight per wave; a step is NT KiB of codes and 5 NT registers). NT = 8 carries 32 x MT
// accumulator registers: 4 steps up to 3 row tiles, 3 at 5, 2 at 7 (the deepest each that compiles without a spill).
constexpr int kMaxMtNt8 = 7;
constexpr int ring_of(int nt, int mt) { return nt == 8 ? (mt <= 3 ? 4 : mt <= 5 ? 3 : 2) : nt == 4 ? 6 : 8; }

int round_mt(int mtiles) {
  static const int kMT[] = {1, 2, 3, 5, 7, 9};
  for (int c : kMT)
    if (c >= mtiles) return c;
  return 0;
}

// Columns per wave (NT) and K split, deterministically from the shape. Model of a launch (us): rounds of 256 workgroups x
// steps x (code bytes of a step / 18.6 GB/s + x bytes of a step / 67 GB/s: the two measured per-CU rates of gemm_wide.hip's
// time model, which ADD) + the pipeline fill per round + the slab traffic of a split (gemm_wide.hip::wide_cost's terms).
// PREDICTED rates for this kernel, not fitted ones: tools/gemm_fp8_bench.py --mxfp4 records what the plans measure.
bool fp4_plan(int64_t m, int n, int k, int mode, Fp4Plan* best) {
  if (m < 1 || m > 256 || n < 16 || k < kBK || k % kBK) return false;
  if (m * (int64_t)k >= (1ll << 31)) return false;                // 32-bit x element offsets in the loader
  if (mode == EPI_SILU ? n % 32 : n % 16) return false;
  const int mtiles = (int)((m + 15) / 16), ksteps = k / kBK;
  Fp4Plan p;
  p.mgroups = mtiles > 9 ? 2 : 1;
  p.mt = round_mt((mtiles + p.mgroups - 1) / p.mgroups);
  const int max_split = mode == EPI_PARTIAL ? 8 : 16;             // (consumers of the slabs take at most 8)
  double best_t = 1e30;
  for (int nt : {8, 4, 2}) {
    if (nt == 8 && p.mt > kMaxMtNt8) continue;
    p.nt = nt;
    const double t_step = kNW * nt * (kTileStep + kScaleStep) / 18.6e3 + p.mt * 16 * 256.0 / 67.0e3;
    for (int split = 1; split <= max_split; ++split) {
      if (ksteps % split || (split > 1 && ksteps / split < 2)) continue;
      p.split = split;
      p.steps = ksteps / split;
      // a split bf16 / SiLU launch tiles all n columns (the reduce kernel forms the SiLU pairs)
      const bool pairs = mode == EPI_SILU && split == 1;
      const int cols = kNW * nt * 16 / (pairs ? 2 : 1), units = pairs ? n / 2 : n;
      p.tiles = (units + cols - 1) / cols;
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
int launch_fp4(const Fp4Plan& p, const void* x, const void* codes, const void* scales, void* out, int64_t m, int n, int k,
               int epi, hipStream_t s) {
  constexpr int RING = ring_of(NT, MT);
  const size_t lds = (size_t)kNS * MT * 16 * kRowB;
  static bool attr_done[NVL_MAX_DEVICES] = {};
  bool& attr_set = attr_done[nvl_device_slot()];
  if (!attr_set && lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&linear_wide_mxfp4_kernel<MT, NT, RING>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      nvl_set_error("nvl_linear_wide_mxfp4: cannot reserve %zu B of LDS", lds);
      return NVL_ELAUNCH;
    }
    attr_set = true;
  }
  const dim3 grid = p.mgroups == 2 ? dim3((unsigned)((p.tiles + 7) / 8) * 16, p.split, 1) : dim3(p.tiles, p.split, 1);
  hipLaunchKernelGGL((linear_wide_mxfp4_kernel<MT, NT, RING>), grid, dim3((kNW + 1) * 64), lds, s, (const bf16_t*)x,
                     (const unsigned char*)codes, (const unsigned char*)scales, out, (int)m, n, k, p.steps, epi,
                     p.mgroups == 2 ? p.tiles : 0);
  return NVL_OK;
}

int dispatch_fp4(const Fp4Plan& p, const void* x, const void* codes, const void* scales, void* out, int64_t m, int n, int k,
                 int epi, hipStream_t s) {
#define NVL_F4(MT_)                                                                                         \
  if (p.mt == MT_) {                                                                                        \
    if constexpr (MT_ <= kMaxMtNt8)                                                                         \
      if (p.nt == 8) return launch_fp4<MT_, 8>(p, x, codes, scales, out, m, n, k, epi, s);                   \
    if (p.nt == 4) return launch_fp4<MT_, 4>(p, x, codes, scales, out, m, n, k, epi, s);                     \
    if (p.nt == 2) return launch_fp4<MT_, 2>(p, x, codes, scales, out, m, n, k, epi, s);                     \
  }
  NVL_F4(1) NVL_F4(2) NVL_F4(3) NVL_F4(5) NVL_F4(7) NVL_F4(9)
#undef NVL_F4
  // (a plan with no instantiation behind it, e.g. 8 column tiles at 9 row tiles, is refused, never remapped)
  nvl_set_error("nvl_linear_wide_mxfp4: internal plan error (mt=%d nt=%d)", p.mt, p.nt);
  return NVL_EINVAL;
}

}  // namespace

extern "C" int nvl_linear_wide_mxfp4_plan(int64_t m, int n, int k, int mode, int* splits, size_t* workspace_bytes) {
  Fp4Plan p;
  if (mode < 0 || mode > 2 || !fp4_plan(m, n, k, mode, &p)) return 0;
  if (splits) *splits = p.split;
  if (workspace_bytes) *workspace_bytes = mode != EPI_PARTIAL && p.split > 1 ? (size_t)p.split * m * n * sizeof(float) : 0;
  return 1;
}

extern "C" int nvl_unpack_mxfp4(const void* codes, const void* scales, void* w_bf16_out, int64_t n, int64_t k, void* stream) {
  NVL_REQUIRE(codes && scales && w_bf16_out, "nvl_unpack_mxfp4: null pointer");
  NVL_REQUIRE(n > 0 && n % 16 == 0, "nvl_unpack_mxfp4: n=%lld must be a positive multiple of 16", (long long)n);
  NVL_REQUIRE(k > 0 && k % 128 == 0, "nvl_unpack_mxfp4: k=%lld must be a positive multiple of 128", (long long)k);
  NVL_REQUIRE(((uintptr_t)codes | (uintptr_t)scales | (uintptr_t)w_bf16_out) % 16 == 0,
              "nvl_unpack_mxfp4: pointers must be 16-byte aligned");
  const int64_t chunks = n * k / 32;                              // 16 bytes of codes = 32 weights each
  NVL_REQUIRE(k / 128 <= (1 << 20) && (chunks + 255) / 256 <= 0x7fffffffLL,
              "nvl_unpack_mxfp4: n=%lld k=%lld is too large for one launch", (long long)n, (long long)k);
  hipLaunchKernelGGL(unpack_mxfp4_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)codes, (const unsigned char*)scales, (bf16_t*)w_bf16_out, chunks, (int)(k / 128), k);
  return nvl_check_launch("nvl_unpack_mxfp4");
}

extern "C" int nvl_linear_wide_mxfp4(const void* x, const void* codes, const void* scales_tiled, void* out, int64_t m, int n,
                                     int k, int mode, void* workspace, size_t workspace_bytes, void* stream) {
  NVL_REQUIRE(x && codes && scales_tiled && out, "nvl_linear_wide_mxfp4: null pointer");
  NVL_REQUIRE(mode >= 0 && mode <= 2, "nvl_linear_wide_mxfp4: mode=%d (0 bf16, 1 silu*mul, 2 split-K fp32 partials)", mode);
  NVL_REQUIRE(((uintptr_t)x | (uintptr_t)codes | (uintptr_t)scales_tiled | (uintptr_t)out | (uintptr_t)workspace) % 16 == 0,
              "nvl_linear_wide_mxfp4: pointers must be 16-byte aligned");
  Fp4Plan p;
  if (!fp4_plan(m, n, k, mode, &p)) {
    nvl_set_error("nvl_linear_wide_mxfp4: shape m=%lld n=%d k=%d mode=%d not covered (query nvl_linear_wide_mxfp4_plan first)",
                  (long long)m, n, k, mode);
    return NVL_EUNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  if (mode == EPI_PARTIAL || p.split == 1) {
    const int rc = dispatch_fp4(p, x, codes, scales_tiled, out, m, n, k, mode, s);
    return rc != NVL_OK ? rc : nvl_check_launch("nvl_linear_wide_mxfp4");
  }
  const size_t need = (size_t)p.split * m * n * sizeof(float);
  NVL_REQUIRE(workspace && workspace_bytes >= need, "nvl_linear_wide_mxfp4: workspace %zu B < required %zu B", workspace_bytes,
              need);
  const int rc = dispatch_fp4(p, x, codes, scales_tiled, workspace, m, n, k, EPI_PARTIAL, s);
  if (rc != NVL_OK) return rc;
  const int out_cols = mode == EPI_SILU ? n / 2 : n;
  const unsigned blocks = (unsigned)((m * (int64_t)(out_cols / 4) + 255) / 256);
  if (mode == EPI_SILU)
    hipLaunchKernelGGL(slab_reduce_mxfp4_kernel<EPI_SILU>, dim3(blocks), dim3(256), 0, s, (const float*)workspace, p.split,
                       (int64_t)m * n, (bf16_t*)out, (int)m, n);
  else
    hipLaunchKernelGGL(slab_reduce_mxfp4_kernel<EPI_BF16>, dim3(blocks), dim3(256), 0, s, (const float*)workspace, p.split,
                       (int64_t)m * n, (bf16_t*)out, (int)m, n);
  return nvl_check_launch("nvl_linear_wide_mxfp4");
}
