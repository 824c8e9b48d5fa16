// Single-pass token sampler for gfx950.
// Replaces Sampler.forward (nano-vllm layers/sampler.py:7-12):
//     argmax_i softmax(l/T)_i / E_i ,  E_i ~ Exp(1), clamp_min 1e-10
// = argmax_i ( l_i/T - log E_i )  — the softmax normaliser is common to the row and cancels,
// so one streaming read of the bf16 logits (2 B/logit) replaces the reference's fp32 [B,V]
// temporaries. E_i comes from Philox4x32-10 keyed by (seed; offset, row, column/4): the draw
// does not depend on grid shape, so host code can replay it (nvl_sample_exponentials_host).
// With `row_keys` (what the engine passes) the "row" of that key is not the batch row but the SEQUENCE:
// row_keys[r] = sequence id | position << 32 -> the draw uses row = low word, offset + high word, i.e. it depends on
// (seed, sequence, position, column) only — not on where the sequence sits in the batch, which step of the engine this
// is, or what else is in flight (lookahead, preemption, other requests).
// T == 0 selects plain argmax (lowest index wins ties), an extension the reference forbids
// (sampling_params.py:11) but the parity harness needs.
#include "common.h"
#include <math.h>

namespace {

constexpr int kSplits = 8;  // workgroups per row

// u in (0,1): 24 random bits, centred.
__host__ __device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

__host__ __device__ __forceinline__ float exp1_from_bits(uint32_t x) {
#ifdef __HIP_DEVICE_COMPILE__
  const float e = -log_normal_f32(u01(x));
#else
  const float e = -logf(u01(x));
#endif
  return e < 1e-10f ? 1e-10f : e;
}

// The race, shared by every sampler kernel of this file. Philox call `call` covers global columns 4 * call .. + 3 of the
// draw at stream offset `off` for sampler row `rowid` (nvl_sample_exponentials_host restates the keying).
__device__ __forceinline__ Philox4 race_draw(int64_t call, uint64_t off, uint32_t rowid, uint32_t k0, uint32_t k1) {
  return philox4x32_10((uint32_t)call, (uint32_t)(call >> 32) ^ (uint32_t)(off << 8), rowid, (uint32_t)(off >> 24), k0, k1);
}
__device__ __forceinline__ float race_key(float l, float invT, uint32_t bits) {
  return l * invT - log_normal_f32(exp1_from_bits(bits));
}

struct Best {
  float v;
  int idx;
};
__device__ __forceinline__ Best better(Best a, Best b) {
  // larger value wins; on ties the lower index (torch.argmax: first maximal value)
  if (b.v > a.v || (b.v == a.v && b.idx < a.idx)) return b;
  return a;
}

__global__ __launch_bounds__(256) void sample_partial_kernel(const bf16_t* __restrict__ logits, int64_t row_stride,
                                                              const float* __restrict__ temps, int64_t vocab,
                                                              int64_t col_offset, uint64_t seed, uint64_t offset,
                                                              const uint64_t* __restrict__ offset_dev,
                                                              const uint64_t* __restrict__ row_keys,
                                                              float* __restrict__ ws_val, int* __restrict__ ws_idx) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int64_t row = blockIdx.y;
  const int split = blockIdx.x;
  const float T = temps[row];
  const bool greedy = !(T > 0.f);
  const float invT = greedy ? 1.f : 1.f / T;
  const uint64_t rk = row_keys ? row_keys[row] : (uint64_t)row;
  const uint32_t rowid = (uint32_t)rk;
  const uint64_t off = offset + (offset_dev ? *offset_dev : 0ull) + (rk >> 32);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const bf16_t* lr = logits + row * row_stride;
  const int64_t nchunks = (vocab + 7) >> 3;
  const int64_t per = (nchunks + kSplits - 1) / kSplits;
  const int64_t c_begin = split * per;
  const int64_t c_end = min(nchunks, c_begin + per);
  Best best{-INFINITY, 0x7fffffff};
  const bool vec_ok = ((reinterpret_cast<uintptr_t>(lr) & 15) == 0);
  // `col_offset` (a multiple of 8) = global vocabulary index of local column 0: a vocab-parallel shard
  // (embed_head.py:56-66) draws the SAME exponentials and reports the SAME indices as the full row would.
  const int64_t gchunk0 = col_offset >> 3;
  for (int64_t c = c_begin + threadIdx.x; c < c_end; c += 256) {
    const int64_t col0 = c * 8;
    const int64_t gc = c + gchunk0;
    float f[8];
    if (vec_ok && col0 + 8 <= vocab) {
      unpack8(*reinterpret_cast<const u32x4_t*>(lr + col0), f);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = (col0 + i < vocab) ? (float)lr[col0 + i] : -INFINITY;
    }
    float key[8];
    if (greedy) {
#pragma unroll
      for (int i = 0; i < 8; ++i) key[i] = f[i];
    } else {
      const Philox4 r0 = race_draw(2 * gc, off, rowid, k0, k1);
      const Philox4 r1 = race_draw(2 * gc + 1, off, rowid, k0, k1);
#pragma unroll
      for (int i = 0; i < 8; ++i) key[i] = race_key(f[i], invT, i < 4 ? r0.v[i] : r1.v[i - 4]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (col0 + i < vocab) best = better(best, Best{key[i], (int)(col_offset + col0 + i)});
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best other{__shfl_xor(best.v, o, 64), __shfl_xor(best.idx, o, 64)};
    best = better(best, other);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sv[wave] = best.v;
    si[wave] = best.idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Best b{sv[0], si[0]};
#pragma unroll
    for (int w = 1; w < 4; ++w) b = better(b, Best{sv[w], si[w]});
    ws_val[row * kSplits + split] = b.v;
    ws_idx[row * kSplits + split] = b.idx;
  }
}

// Merge `parts` (value, index) partials per row: part p of row r lives at val[p * part_stride + r * inner + j],
// j < inner (inner = kSplits for the workgroup partials of one launch, 1 for per-rank results). Either writes the
// winning index (int64, what Sampler.forward returns) or the packed {value bits, index} pair of a shard.
__global__ __launch_bounds__(64) void sample_merge_kernel(const float* __restrict__ val, const int* __restrict__ idx,
                                                           int parts, int64_t part_stride, int inner,
                                                           int64_t* __restrict__ out, uint32_t* __restrict__ out_packed,
                                                           int64_t batch) {
  const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= batch) return;
  Best b{-INFINITY, 0x7fffffff};
  for (int p = 0; p < parts; ++p)
    for (int j = 0; j < inner; ++j) {
      const int64_t at = p * part_stride + row * inner + j;
      b = better(b, Best{val[at], idx[at]});
    }
  if (out) out[row] = b.idx == 0x7fffffff ? 0 : (int64_t)b.idx;
  if (out_packed) {
    out_packed[row * 2] = __float_as_uint(b.v);
    out_packed[row * 2 + 1] = (uint32_t)b.idx;
  }
}

// packed {value bits, index} pairs [parts][batch][2] (one part per tensor-parallel rank) -> winning index
__global__ __launch_bounds__(64) void sample_merge_packed_kernel(const uint32_t* __restrict__ packed, int parts,
                                                                  int64_t part_stride_words, int64_t* __restrict__ out,
                                                                  int64_t batch) {
  const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= batch) return;
  Best b{-INFINITY, 0x7fffffff};
  for (int p = 0; p < parts; ++p) {
    const uint32_t* q = packed + p * part_stride_words + row * 2;
    b = better(b, Best{__uint_as_float(q[0]), (int)q[1]});
  }
  out[row] = b.idx == 0x7fffffff ? 0 : (int64_t)b.idx;
}

// ---- Top-k / top-p: exact radix select over the 16-bit order key of bf16, then the same race over the kept set --------
// One 1024-thread workgroup per row. A filtered row is read from memory ONCE into registers (NCH 16-byte chunks per lane:
// 19 x 1024 x 8 = 155,648 columns cover the Qwen3 vocabulary in 76 of the 128 registers a lane has at 16 waves per CU) and
// every selection pass walks the registers:
//   max -> [top-k] count histogram of the key's high byte, of its low byte inside the bin of the k-th element  => v_k
//       -> [top-p] mass histogram of the keys >= v_k by high byte, by low byte inside the bin of the quantile => v_p
//       -> the columns with key >= tau go to a list in LDS; the race draws Philox for those columns only.
// Histograms are 256 bins x 16 copies of u64 in LDS (copy = lane & 15: a hot bin — the logits of a row share a handful of
// exponents — is hit by 4 lanes of a wave instead of 64). Counts and masses are both integers (mass = round(w * 2^40),
// w = exp((l - max) / T) <= 1, at most 2^58 per row), so a sum does not depend on the order of its atomics and tau is the
// same on every run. Rows without a filter, greedy rows and kept sets too long for the list take the full-row race from
// memory — the plain kernel's loop with a key threshold — and return nvl_sample's token bit for bit.
// NCH = 0: a row too long for the registers is re-read from memory (L2 / Infinity Cache by then) in every pass.
constexpr int kSelThreads = 1024;
constexpr int kSelCopies = 16;
constexpr int kSelListCap = 2048;
constexpr uint32_t kKeyNegInf = 0x007fu;    // order_key(-inf): every finite value is above, every negative NaN below
constexpr uint32_t kPadWord = 0xffffffffu;  // two bf16 NaN patterns with order key 0: columns past the end of the row

// bf16 bits -> 16-bit key whose unsigned order is the order of the values (-0 counts as +0: they are equal)
__device__ __forceinline__ uint32_t order_key(uint32_t b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ float order_key_value(uint32_t key) {
  const uint32_t b = (key & 0x8000u) ? (key ^ 0x8000u) : (~key & 0xffffu);
  return __uint_as_float(b << 16);
}

// 16-byte chunk c of a row as raw bf16 pairs; columns >= vocab read as padding
__device__ __forceinline__ u32x4_t load_chunk_bits(const uint16_t* __restrict__ lr, int64_t vocab, bool vec_ok, int64_t c) {
  const int64_t col0 = c * 8;
  if (vec_ok && col0 + 8 <= vocab) return *reinterpret_cast<const u32x4_t*>(lr + col0);
  u32x4_t w;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t lo = (col0 + 2 * i < vocab) ? lr[col0 + 2 * i] : 0xffffu;
    const uint32_t hi = (col0 + 2 * i + 1 < vocab) ? lr[col0 + 2 * i + 1] : 0xffffu;
    w[i] = lo | (hi << 16);
  }
  return w;
}

template <class F>
__device__ __forceinline__ void visit_chunk(const u32x4_t& w, int col0, F& f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f(order_key(w[i] & 0xffffu), col0 + 2 * i);
    f(order_key(w[i] >> 16), col0 + 2 * i + 1);
  }
}

// f(order key, column) for every column of the row (padding columns come with key 0). The empty asm statement keeps the
// compiler from carrying the 8 x NCH unpacked keys (or their weights) from one pass to the next: the packed words are what
// stays resident, a pass unpacks them again.
template <int NCH, class F>
__device__ __forceinline__ void for_each_key(u32x4_t (&regs)[NCH > 0 ? NCH : 1], const uint16_t* __restrict__ lr,
                                             int64_t vocab, bool vec_ok, F f) {
  if constexpr (NCH > 0) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      asm volatile("" : "+v"(regs[j]));
      visit_chunk(regs[j], ((int)threadIdx.x + j * kSelThreads) * 8, f);
    }
  } else {
    const int64_t nchunks = (vocab + 7) >> 3;
    for (int64_t c = threadIdx.x; c < nchunks; c += kSelThreads) visit_chunk(load_chunk_bits(lr, vocab, vec_ok, c), (int)(c * 8), f);
  }
}

struct Cut {
  uint32_t bin;                     // first bin from the top at which the running sum reaches the target
  unsigned long long above, target; // sum of the bins above it; the target used
};
// Wave 0: top-down scan of tot[256]. `frac` >= 0: target = frac x (sum of all bins), else `target` as given.
__device__ __forceinline__ Cut scan_from_top(const unsigned long long* tot, unsigned long long target, float frac) {
  const int lane = threadIdx.x & 63;
  unsigned long long s[4], sum = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s[i] = tot[255 - (4 * lane + i)];
    sum += s[i];
  }
  unsigned long long incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  const unsigned long long total = __shfl(incl, 63, 64);
  if (frac >= 0.f) target = (unsigned long long)((double)frac * (double)total);
  if (target > total) target = total;
  if (target < 1) target = 1;
  const unsigned long long hit = __ballot(incl >= target);
  const int first = hit ? __ffsll((long long)hit) - 1 : 63;
  unsigned long long run = incl - sum;
  uint32_t bin = 255 - (4 * lane + 3);
  bool found = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!found) {
      if (run + s[i] >= target || i == 3) {
        bin = 255 - (4 * lane + i);
        found = true;
      } else {
        run += s[i];
      }
    }
  }
  Cut c;
  c.bin = __shfl(bin, first, 64);
  c.above = __shfl(run, first, 64);
  c.target = target;
  return c;
}

// A value every lane read from the same LDS word, moved to scalar registers (the resident row leaves ~50 vector ones).
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);      // (the builtin returns a signed int)
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}
__device__ __forceinline__ Cut uniform_cut(const Cut& c) {
  return Cut{(uint32_t)__builtin_amdgcn_readfirstlane(c.bin), uniform_u64(c.above), uniform_u64(c.target)};
}

template <int NCH>
__global__ __launch_bounds__(kSelThreads) void sample_select_kernel(
    const bf16_t* __restrict__ logits, int64_t row_stride, const float* __restrict__ temps,
    const int32_t* __restrict__ top_k, const float* __restrict__ top_p, int64_t vocab, uint64_t seed, uint64_t offset,
    const uint64_t* __restrict__ offset_dev, const uint64_t* __restrict__ row_keys, int64_t* __restrict__ out,
    float* __restrict__ tau_out) {
  __shared__ unsigned long long hist[256 * kSelCopies];
  __shared__ unsigned long long tot[256];
  __shared__ uint32_t list[kSelListCap];
  __shared__ uint32_t su[kSelThreads / 64];
  __shared__ float sv[kSelThreads / 64];
  __shared__ int si[kSelThreads / 64];
  __shared__ Cut s_cut;
  __shared__ uint32_t s_n;

  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float T = temps[row];
  const bool greedy = !(T > 0.f);
  // (the division runs on the vector unit: back to a scalar register, the resident row leaves few vector ones)
  const float invT = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(greedy ? 1.f : 1.f / T)));
  const int32_t k = top_k[row];
  const float p = top_p[row];
  const bool k_on = k > 0 && k < vocab, p_on = p < 1.f;
  const uint64_t rk = row_keys ? row_keys[row] : (uint64_t)row;
  const uint32_t rowid = (uint32_t)rk;
  const uint64_t off = offset + (offset_dev ? *offset_dev : 0ull) + (rk >> 32);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const bf16_t* lrow = logits + row * row_stride;
  const uint16_t* lr = reinterpret_cast<const uint16_t*>(lrow);
  const bool vec_ok = ((reinterpret_cast<uintptr_t>(lr) & 15) == 0);
  const int64_t nchunks = (vocab + 7) >> 3;

  uint32_t tkey = 0;          // keep the columns whose order key is >= tkey (0: every column)
  // A filter that asks for ONE column (top_k == 1, or one maximal column already holds top_p of the mass) makes the row
  // greedy: the maxima are what is kept, and as for T == 0 the lowest index among them is the token, not a draw.
  bool pick_max = greedy;
  bool use_list = false;
  uint32_t nlist = 0;
  if (!greedy && (k_on || p_on)) {
    u32x4_t regs[NCH > 0 ? NCH : 1];
    if constexpr (NCH > 0) {
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int64_t c = tid + j * kSelThreads;
        regs[j] = c < nchunks ? load_chunk_bits(lr, vocab, vec_ok, c) : u32x4_t{kPadWord, kPadWord, kPadWord, kPadWord};
      }
    }
    // row maximum (as a key)
    uint32_t kmax = 0;
    for_each_key<NCH>(regs, lr, vocab, vec_ok, [&](uint32_t key, int) { kmax = max(kmax, key); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
    if (lane == 0) su[wave] = kmax;
    if (tid == 0) s_n = 0;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kSelThreads / 64; ++w) kmax = max(kmax, su[w]);
    kmax = __builtin_amdgcn_readfirstlane(kmax);
    if (kmax <= kKeyNegInf) {     // the whole row is -inf: token 0, as the plain sampler
      if (tid == 0) {
        out[row] = 0;
        if (tau_out) tau_out[row] = -INFINITY;
      }
      return;
    }
    const float vmax = order_key_value(kmax);
    // 2^40 x the weight of a key, rounded to an integer
    auto mass = [&](uint32_t key) -> unsigned long long {
      return (unsigned long long)__float2ull_rn(__expf((order_key_value(key) - vmax) * invT) * 1099511627776.f);
    };
    // one histogram pass: add(key) -> (bin, amount) for the keys that count, then the scan for `target` / `frac`
    auto select = [&](auto add, unsigned long long target, float frac) -> Cut {
      for (int i = tid; i < 256 * kSelCopies; i += kSelThreads) hist[i] = 0;
      __syncthreads();
      for_each_key<NCH>(regs, lr, vocab, vec_ok, [&](uint32_t key, int) {
        uint32_t bin;
        unsigned long long amount;
        if (add(key, bin, amount)) atomicAdd(&hist[bin * kSelCopies + (lane & (kSelCopies - 1))], amount);
      });
      __syncthreads();
      if (tid < 256) {
        unsigned long long s = 0;
#pragma unroll
        for (int c = 0; c < kSelCopies; ++c) s += hist[tid * kSelCopies + ((c + tid) & (kSelCopies - 1))];
        tot[tid] = s;
      }
      __syncthreads();
      if (wave == 0) {
        const Cut c = scan_from_top(tot, target, frac);
        if (lane == 0) s_cut = c;
      }
      __syncthreads();
      return uniform_cut(s_cut);
    };

    tkey = kKeyNegInf;
    if (k_on) {
      const Cut hi = select([&](uint32_t key, uint32_t& bin, unsigned long long& amount) {
        bin = key >> 8, amount = 1;
        return key != 0;
      }, (unsigned long long)k, -1.f);
      const Cut lo = select([&](uint32_t key, uint32_t& bin, unsigned long long& amount) {
        bin = key & 0xffu, amount = 1;
        return key != 0 && (key >> 8) == hi.bin;
      }, (unsigned long long)k - hi.above, -1.f);
      tkey = max((hi.bin << 8) | lo.bin, kKeyNegInf);
      pick_max = k == 1;
    }
    if (p_on) {
      const uint32_t from = max(tkey, kKeyNegInf + 1);      // -inf columns weigh nothing
      const Cut hi = select([&](uint32_t key, uint32_t& bin, unsigned long long& amount) {
        if (key < from) return false;
        bin = key >> 8, amount = mass(key);
        return true;
      }, 0, p);
      const Cut lo = select([&](uint32_t key, uint32_t& bin, unsigned long long& amount) {
        if (key < from || (key >> 8) != hi.bin) return false;
        bin = key & 0xffu, amount = mass(key);
        return true;
      }, hi.target - hi.above, -1.f);
      tkey = max((hi.bin << 8) | lo.bin, from);
      pick_max = pick_max || hi.target <= (1ull << 40);      // the weight of a maximal column is exactly 2^40
    }
    // the kept columns -> list, when they fit
    uint32_t mine = 0;
    for_each_key<NCH>(regs, lr, vocab, vec_ok, [&](uint32_t key, int) { mine += key >= tkey ? 1u : 0u; });
    uint32_t kept = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += (uint32_t)__shfl_xor((int)kept, o, 64);
    if (lane == 0) su[wave] = kept;
    __syncthreads();
    kept = 0;
#pragma unroll
    for (int w = 0; w < kSelThreads / 64; ++w) kept += su[w];
    use_list = kept <= (uint32_t)kSelListCap;
    if (use_list) {
      uint32_t at = mine ? atomicAdd(&s_n, mine) : 0u;
      for_each_key<NCH>(regs, lr, vocab, vec_ok, [&](uint32_t key, int col) {
        if (key >= tkey && at < (uint32_t)kSelListCap) list[at++] = (uint32_t)col;
      });
      nlist = kept;
    }
    __syncthreads();
  }

  Best best{-INFINITY, 0x7fffffff};
  if (use_list) {
    for (uint32_t e = tid; e < nlist; e += kSelThreads) {
      const int col = (int)list[e];
      const Philox4 r = race_draw((int64_t)(col >> 2), off, rowid, k0, k1);
      const int q = col & 3;      // (selects: a variable index would put r.v in memory)
      const uint32_t bits = q == 0 ? r.v[0] : q == 1 ? r.v[1] : q == 2 ? r.v[2] : r.v[3];
      const float l = (float)lrow[col];
      best = better(best, Best{pick_max ? l : race_key(l, invT, bits), col});
    }
  } else {
    // full-row race: the plain kernel's loop, over the columns with key >= tkey
    for (int64_t c = tid; c < nchunks; c += kSelThreads) {
      const u32x4_t w = load_chunk_bits(lr, vocab, vec_ok, c);
      const int64_t col0 = c * 8;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float f[4];
        bool keep[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t b = (i & 1) ? (w[2 * h + (i >> 1)] >> 16) : (w[2 * h + (i >> 1)] & 0xffffu);
          f[i] = __uint_as_float(b << 16);
          keep[i] = col0 + 4 * h + i < vocab && order_key(b) >= tkey;
        }
        if (pick_max) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (keep[i]) best = better(best, Best{f[i], (int)(col0 + 4 * h + i)});
        } else if (keep[0] || keep[1] || keep[2] || keep[3]) {
          const Philox4 r = race_draw(2 * c + h, off, rowid, k0, k1);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (keep[i]) best = better(best, Best{race_key(f[i], invT, r.v[i]), (int)(col0 + 4 * h + i)});
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best other{__shfl_xor(best.v, o, 64), __shfl_xor(best.idx, o, 64)};
    best = better(best, other);
  }
  if (lane == 0) {
    sv[wave] = best.v;
    si[wave] = best.idx;
  }
  __syncthreads();
  if (tid == 0) {
    Best b{sv[0], si[0]};
#pragma unroll
    for (int w = 1; w < kSelThreads / 64; ++w) b = better(b, Best{sv[w], si[w]});
    out[row] = b.idx == 0x7fffffff ? 0 : (int64_t)b.idx;
    if (tau_out) tau_out[row] = tkey > kKeyNegInf ? order_key_value(tkey) : -INFINITY;
  }
}

}  // namespace

extern "C" size_t nvl_sample_workspace_bytes(int64_t max_batch) {
  if (max_batch <= 0) return 0;
  return (size_t)max_batch * kSplits * (sizeof(float) + sizeof(int));
}

namespace {
int sample_common(const void* logits, int64_t logits_row_stride, const float* temperatures, int64_t* out,
                  uint32_t* out_packed, int64_t batch, int64_t vocab, int64_t col_offset, uint64_t seed, uint64_t offset,
                  const uint64_t* offset_dev, const uint64_t* row_keys, void* workspace, size_t workspace_bytes,
                  void* stream, const char* who) {
  NVL_REQUIRE(logits && temperatures && (out || out_packed) && workspace, "%s: null pointer", who);
  NVL_REQUIRE(batch >= 0 && batch <= 65535, "%s: batch=%lld out of range [0, 65535]", who, (long long)batch);
  NVL_REQUIRE(vocab > 0 && col_offset >= 0 && col_offset + vocab < (1ll << 31) - 8, "%s: bad vocab=%lld (+%lld)", who,
              (long long)vocab, (long long)col_offset);
  NVL_REQUIRE(col_offset % 8 == 0, "%s: col_offset=%lld must be a multiple of 8", who, (long long)col_offset);
  NVL_REQUIRE(logits_row_stride >= vocab, "%s: row stride < vocab", who);
  NVL_REQUIRE(workspace_bytes >= nvl_sample_workspace_bytes(batch), "%s: workspace too small", who);
  NVL_REQUIRE(((uintptr_t)workspace) % 8 == 0, "%s: workspace must be 8-byte aligned", who);
  if (batch == 0) return NVL_OK;
  float* ws_val = (float*)workspace;
  int* ws_idx = (int*)(ws_val + (size_t)batch * kSplits);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sample_partial_kernel, dim3(kSplits, (unsigned)batch), dim3(256), 0, s, (const bf16_t*)logits,
                     logits_row_stride, temperatures, vocab, col_offset, seed, offset, offset_dev, row_keys, ws_val, ws_idx);
  hipLaunchKernelGGL(sample_merge_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, ws_val, ws_idx, 1,
                     (int64_t)0, kSplits, out, out_packed, batch);
  return nvl_check_launch(who);
}
}  // namespace

extern "C" int nvl_sample(const void* logits, int64_t logits_row_stride, const float* temperatures, int64_t* out,
                          int64_t batch, int64_t vocab, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                          const uint64_t* row_keys, void* workspace, size_t workspace_bytes, void* stream) {
  return sample_common(logits, logits_row_stride, temperatures, out, nullptr, batch, vocab, 0, seed, offset,
                       offset_dev, row_keys, workspace, workspace_bytes, stream, "nvl_sample");
}

extern "C" int nvl_sample_shard(const void* logits, int64_t logits_row_stride, const float* temperatures,
                                void* best_packed, int64_t batch, int64_t vocab_local, int64_t col_offset,
                                uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                                const uint64_t* row_keys, void* workspace, size_t workspace_bytes, void* stream) {
  NVL_REQUIRE(((uintptr_t)best_packed) % 8 == 0, "nvl_sample_shard: best_packed must be 8-byte aligned");
  return sample_common(logits, logits_row_stride, temperatures, nullptr, (uint32_t*)best_packed, batch, vocab_local,
                       col_offset, seed, offset, offset_dev, row_keys, workspace, workspace_bytes, stream,
                       "nvl_sample_shard");
}

extern "C" int nvl_sample_merge(const void* best_packed, int parts, int64_t part_stride_bytes, int64_t* out,
                                int64_t batch, void* stream) {
  NVL_REQUIRE(best_packed && out, "nvl_sample_merge: null pointer");
  NVL_REQUIRE(parts >= 1 && parts <= 1024, "nvl_sample_merge: parts=%d out of range", parts);
  NVL_REQUIRE(batch >= 0 && batch <= 65535, "nvl_sample_merge: batch=%lld out of range", (long long)batch);
  NVL_REQUIRE(part_stride_bytes % 8 == 0 && part_stride_bytes >= batch * 8, "nvl_sample_merge: bad part stride");
  NVL_REQUIRE(((uintptr_t)best_packed) % 8 == 0, "nvl_sample_merge: best_packed must be 8-byte aligned");
  if (batch == 0) return NVL_OK;
  hipLaunchKernelGGL(sample_merge_packed_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                     (const uint32_t*)best_packed, parts, part_stride_bytes / 4, out, batch);
  return nvl_check_launch("nvl_sample_merge");
}

extern "C" int nvl_sample_topk_topp(const void* logits, int64_t logits_row_stride, const float* temperatures,
                                    const int32_t* top_k, const float* top_p, int64_t* out, float* tau, int64_t batch,
                                    int64_t vocab, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                                    const uint64_t* row_keys, void* stream) {
  const char* who = "nvl_sample_topk_topp";
  NVL_REQUIRE(logits && temperatures && top_k && top_p && out, "%s: null pointer", who);
  NVL_REQUIRE(batch >= 0 && batch <= 65535, "%s: batch=%lld out of range [0, 65535]", who, (long long)batch);
  NVL_REQUIRE(vocab > 0 && vocab < (1ll << 31) - 8, "%s: bad vocab=%lld", who, (long long)vocab);
  NVL_REQUIRE(logits_row_stride >= vocab, "%s: row stride < vocab", who);
  if (batch == 0) return NVL_OK;
  // chunks of 8 columns per lane: the row stays in registers up to 19 (155,648 columns: 76 of a lane's 128 registers)
  const int64_t per_lane = ((vocab + 7) / 8 + kSelThreads - 1) / kSelThreads;
  auto kernel = per_lane <= 5 ? sample_select_kernel<5> : per_lane <= 19 ? sample_select_kernel<19> : sample_select_kernel<0>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(kSelThreads), 0, (hipStream_t)stream, (const bf16_t*)logits,
                     logits_row_stride, temperatures, top_k, top_p, vocab, seed, offset, offset_dev, row_keys, out, tau);
  return nvl_check_launch(who);
}

namespace {
__global__ __launch_bounds__(256) void feed_tokens_kernel(int64_t* __restrict__ ids, const int32_t* __restrict__ src,
                                                          const int64_t* __restrict__ prev, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int32_t r = src[i];
    if (r >= 0) ids[i] = prev[r];
  }
}
}  // namespace

extern "C" int nvl_feed_tokens(int64_t* ids, const int32_t* src_row, const int64_t* prev_tokens, int64_t n,
                               void* stream) {
  NVL_REQUIRE(ids && src_row && prev_tokens, "nvl_feed_tokens: null pointer");
  NVL_REQUIRE(n >= 0 && n < (1ll << 31), "nvl_feed_tokens: bad n=%lld", (long long)n);
  if (n == 0) return NVL_OK;
  hipLaunchKernelGGL(feed_tokens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ids,
                     src_row, prev_tokens, n);
  return nvl_check_launch("nvl_feed_tokens");
}

extern "C" void nvl_sample_exponentials_host(uint64_t seed, uint64_t offset, int64_t row, int64_t col0, int64_t n,
                                             float* e_host) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int64_t j = 0; j < n; ++j) {
    const int64_t col = col0 + j;
    const int64_t ctr = col >> 2;  // one Philox call per 4 columns: call index = 2*(col/8) + (col%8)/4
    const Philox4 r = philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32) ^ (uint32_t)(offset << 8), (uint32_t)row,
                                    (uint32_t)(offset >> 24), k0, k1);
    e_host[j] = exp1_from_bits(r.v[col & 3]);
  }
}
