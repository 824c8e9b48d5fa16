// Presence / frequency / repetition penalties on the bf16 logits of a step, from a token history that lives on the device.
//
// The history is a TOKEN CACHE that shadows the paged KV cache: int32 [num_blocks * block_size], entry `slot` = the id of
// the token whose K/V sit at KV slot `slot`. Whatever the block manager does to K/V (prefix-cache hits, preemption and
// recompute, eviction) it does to the token ids as well, so a row's history is its block table, read as
// token_cache[bt[p / bs] * bs + p % bs] for p < context_len. Two writers keep it current: store_tokens_kernel (prefill:
// the step's staged ids and slots) and feed_store_tokens_kernel (decode: nvl_feed_tokens' copy and the store of the
// resolved id in ONE launch, the first node of the captured step).
//
// penalty_apply_kernel: one 1024-thread workgroup per row and table cycle.
//   * a row with all penalties off, or context 0 (graph padding), leaves before touching LDS;
//   * the row's token list is read ONCE, into registers: lane t holds positions t, t + 1024, ... (16 at most: that and the
//     count field below bound max_context at 16,383). The 16 block-table reads are issued back to back, then the 16
//     dependent token reads — coalesced 4-byte loads, all in flight together;
//   * a table of 16-bit fields over the vocabulary lives in LDS, two fields per dword:
//         bits 0-13  count of the token among the OUTPUT positions (p >= prompt_len), LDS atomic add
//         bit  14    always 0: the guard between a count and the flag
//         bit  15    "done": claimed by the thread that rewrites the column
//     a count is at most context_len <= 16,383 = 2^14 - 1: it cannot carry into bit 14, let alone into the neighbour.
//     (There is no "seen" bit to keep: a token that is in the row's list IS seen, and only listed tokens are rewritten —
//     prompt positions cost no atomic at all);
//   * 77,824 fields (152 KiB of the CU's 160) make one table; a longer vocabulary (Qwen3: 151,936) takes a second table
//     cycle over columns 77,824 ..., run by a second workgroup of the row (blockIdx.y) that reads the same list and
//     keeps the tokens of its half: the two halves of a row proceed side by side, neither waits for the other;
//   * the vocabulary is never swept: the token list is walked a second time, the thread that sets a column's done bit
//     first (the atomic's old value tells) reads the final count, loads that one logit, applies the fixed fp32 sequence
//     (no contraction) and stores the rounded bf16. A row reads and writes at most context_len logits.
// Counts are integers and every touched column is written once by one thread from final counts: the result does not
// depend on the order of the atomics and is the same bit for bit on every run. Columns the row never produced keep
// their bits. Ids outside [0, vocab), block ids < 0 and slots past the cache are skipped, never dereferenced.
#include "common.h"

namespace {

constexpr int kPenThreads = 1024;
constexpr int kPenPerLane = 16;                                   // positions of a row one lane holds in registers
constexpr int kPenGroup = 4;                                      // ... handled together (4,096 positions of the row)
constexpr int kPenMaxContext = kPenThreads * kPenPerLane - 1;     // 16,383: also the largest count a field holds
constexpr int kPenFields = 77824;                                 // fields of one table cycle (152 KiB)
constexpr int64_t kPenMaxVocab = 2 * (int64_t)kPenFields;         // 155,648: the top-k / top-p kernel's bound
constexpr uint32_t kCountMask = 0x3fffu, kDoneBit = 0x8000u;
constexpr size_t kPenSpare = 64 * 4;                              // a dword per lane of a wave behind the table


__global__ __launch_bounds__(256) void store_tokens_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ slots,
                                                           int32_t* __restrict__ cache, int64_t cache_slots, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int32_t s = slots[i];
    if (s >= 0 && s < cache_slots) cache[s] = (int32_t)ids[i];
  }
}

__global__ __launch_bounds__(256) void feed_store_tokens_kernel(int64_t* __restrict__ ids, const int32_t* __restrict__ src,
                                                                const int64_t* __restrict__ prev,
                                                                const int32_t* __restrict__ slots,
                                                                int32_t* __restrict__ cache, int64_t cache_slots, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int32_t r = src[i];
    const int64_t id = r >= 0 ? prev[r] : ids[i];
    if (r >= 0) ids[i] = id;
    const int32_t s = slots[i];
    if (s >= 0 && s < cache_slots) cache[s] = (int32_t)id;
  }
}

__global__ __launch_bounds__(kPenThreads) void penalty_apply_kernel(
    bf16_t* __restrict__ logits, int64_t row_stride, const int32_t* __restrict__ cache, int64_t cache_slots,
    const int32_t* __restrict__ block_tables, int64_t bt_stride, int max_blocks, const int32_t* __restrict__ context_lens,
    const int32_t* __restrict__ prompt_lens, const float* __restrict__ presence, const float* __restrict__ frequency,
    const float* __restrict__ repetition, int vocab, int bs_shift, int max_context) {
  extern __shared__ uint32_t table[];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const float pp = presence[row], fp = frequency[row], rp = repetition[row];
  int ctx = context_lens[row];
  if (ctx <= 0 || (pp == 0.f && fp == 0.f && rp == 1.f)) return;
  ctx = min(ctx, min(max_context, kPenMaxContext));
  if ((int64_t)ctx > ((int64_t)max_blocks << bs_shift)) ctx = (int)((int64_t)max_blocks << bs_shift);
  const int plen = prompt_lens[row];
  const int32_t* bt = block_tables + row * bt_stride;
  const int bs_mask = (1 << bs_shift) - 1;

  // the row's token list -> registers (-1: nothing at this position), in groups of kPenGroup registers per lane: a
  // group the context does not reach is skipped by a scalar branch, everything inside a group is branch-free (clamped
  // loads, atomics of lanes with nothing to do go to a spare dword per lane behind the table), so the loads and the
  // atomics of a group are in flight together and no execution mask has to be parked anywhere.
  int32_t tok[kPenPerLane];
#pragma unroll
  for (int g = 0; g < kPenPerLane; g += kPenGroup) {
#pragma unroll
    for (int k = g; k < g + kPenGroup; ++k) tok[k] = -1;
    if (g * kPenThreads < ctx) {
      int32_t blk[kPenGroup];
#pragma unroll
      for (int k = g; k < g + kPenGroup; ++k) blk[k - g] = bt[min(tid + k * kPenThreads, ctx - 1) >> bs_shift];
#pragma unroll
      for (int k = g; k < g + kPenGroup; ++k) {
        const int p = tid + k * kPenThreads;
        const int64_t slot = ((int64_t)blk[k - g] << bs_shift) + (p & bs_mask);
        const bool ok = p < ctx && blk[k - g] >= 0 && slot < cache_slots;
        const int32_t t = cache[ok ? slot : 0];
        tok[k] = ok && (uint32_t)t < (uint32_t)vocab ? t : -1;
      }
    }
  }

  uint16_t* lr = reinterpret_cast<uint16_t*>(logits + row * row_stride);
  {
    const int base = blockIdx.y * kPenFields;                     // this workgroup's table cycle
    const int fields = min(kPenFields, vocab - base);
    const int groups = (fields + 7) >> 3;                         // 16-byte groups of the table; the spare dwords follow
    const uint32_t spare = (uint32_t)groups * 4 + (tid & 63);
    // phase 0: zero the table
    {
      u32x4_t* t4 = reinterpret_cast<u32x4_t*>(table);
      for (int i = tid; i < groups; i += kPenThreads) t4[i] = u32x4_t{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    // phase 1: counts over the output positions
#pragma unroll
    for (int g = 0; g < kPenPerLane; g += kPenGroup) {
      if (g * kPenThreads < ctx) {
#pragma unroll
        for (int k = g; k < g + kPenGroup; ++k) {
          const uint32_t t = (uint32_t)(tok[k] - base);           // (-1 wraps to something no table holds)
          const bool hit = t < (uint32_t)fields && tid + k * kPenThreads >= plen;
          atomicAdd(&table[hit ? t >> 1 : spare], hit ? 1u << ((t & 1) << 4) : 0u);
        }
      }
    }
    __syncthreads();
    // phase 2: the first thread to claim a column rewrites it from the final field
#pragma unroll
    for (int g = 0; g < kPenPerLane; g += kPenGroup) {
      if (g * kPenThreads < ctx) {
        int32_t cnt[kPenGroup];                                   // the claimed column's count, -1: not mine
        uint32_t bits[kPenGroup];
#pragma unroll
        for (int k = g; k < g + kPenGroup; ++k) {
          const uint32_t t = (uint32_t)(tok[k] - base);
          const bool hit = t < (uint32_t)fields;
          const int sh = (t & 1) << 4;
          const uint32_t old = atomicOr(&table[hit ? t >> 1 : spare], hit ? kDoneBit << sh : 0u) >> sh;
          cnt[k - g] = hit && !(old & kDoneBit) ? (int32_t)(old & kCountMask) : -1;
        }
#pragma unroll
        for (int k = g; k < g + kPenGroup; ++k) bits[k - g] = lr[cnt[k - g] >= 0 ? (uint32_t)tok[k] : 0u];
#pragma unroll
        for (int k = g; k < g + kPenGroup; ++k) {
#pragma clang fp contract(off)
          const float c = (float)cnt[k - g];
          float x = __uint_as_float(bits[k - g] << 16);
          x = x > 0.f ? x / rp : x * rp;                          // (a token of the list is seen)
          x = x - fp * c;
          x = x - (c > 0.f ? pp : 0.f);
          if (cnt[k - g] >= 0) lr[(uint32_t)tok[k]] = __builtin_bit_cast(uint16_t, (bf16_t)x);
        }
      }
    }
  }
}

}  // namespace

extern "C" int nvl_store_tokens(const int64_t* ids, const int32_t* slots, int32_t* token_cache, int64_t cache_slots,
                                int64_t n, void* stream) {
  NVL_REQUIRE(ids && slots && token_cache, "nvl_store_tokens: null pointer");
  NVL_REQUIRE(n >= 0 && n < (1ll << 31), "nvl_store_tokens: bad n=%lld", (long long)n);
  NVL_REQUIRE(cache_slots > 0 && cache_slots < (1ll << 31), "nvl_store_tokens: cache_slots=%lld out of range (0, 2^31)",
              (long long)cache_slots);
  if (n == 0) return NVL_OK;
  hipLaunchKernelGGL(store_tokens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ids, slots,
                     token_cache, cache_slots, n);
  return nvl_check_launch("nvl_store_tokens");
}

extern "C" int nvl_feed_store_tokens(int64_t* ids, const int32_t* src_row, const int64_t* prev_tokens, const int32_t* slots,
                                     int32_t* token_cache, int64_t cache_slots, int64_t n, void* stream) {
  NVL_REQUIRE(ids && src_row && prev_tokens && slots && token_cache, "nvl_feed_store_tokens: null pointer");
  NVL_REQUIRE(n >= 0 && n < (1ll << 31), "nvl_feed_store_tokens: bad n=%lld", (long long)n);
  NVL_REQUIRE(cache_slots > 0 && cache_slots < (1ll << 31), "nvl_feed_store_tokens: cache_slots=%lld out of range (0, 2^31)",
              (long long)cache_slots);
  if (n == 0) return NVL_OK;
  hipLaunchKernelGGL(feed_store_tokens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ids,
                     src_row, prev_tokens, slots, token_cache, cache_slots, n);
  return nvl_check_launch("nvl_feed_store_tokens");
}

extern "C" int nvl_apply_penalties(void* logits, int64_t logits_row_stride, const int32_t* token_cache, int64_t cache_slots,
                                   const int32_t* block_tables, int64_t bt_stride, int max_blocks,
                                   const int32_t* context_lens, const int32_t* prompt_lens, const float* presence,
                                   const float* frequency, const float* repetition, int64_t batch, int64_t vocab,
                                   int block_size, int64_t max_context, void* stream) {
  const char* who = "nvl_apply_penalties";
  NVL_REQUIRE(logits && token_cache && block_tables && context_lens && prompt_lens && presence && frequency && repetition,
              "%s: null pointer", who);
  NVL_REQUIRE(batch >= 0 && batch <= 65535, "%s: batch=%lld out of range [0, 65535]", who, (long long)batch);
  NVL_REQUIRE(vocab > 0 && vocab <= kPenMaxVocab, "%s: vocab=%lld out of range (0, %lld]", who, (long long)vocab,
              (long long)kPenMaxVocab);
  NVL_REQUIRE(logits_row_stride >= vocab, "%s: row stride < vocab", who);
  NVL_REQUIRE(block_size > 0 && (block_size & (block_size - 1)) == 0, "%s: block_size=%d is not a power of two", who,
              block_size);
  NVL_REQUIRE(max_context >= 1 && max_context <= kPenMaxContext,
              "%s: max_context=%lld out of range [1, %d] (a 14-bit count per token)", who, (long long)max_context,
              kPenMaxContext);
  NVL_REQUIRE(max_blocks >= 1 && bt_stride >= max_blocks, "%s: bad block table shape (max_blocks=%d, stride=%lld)", who,
              max_blocks, (long long)bt_stride);
  NVL_REQUIRE(cache_slots > 0 && cache_slots < (1ll << 31), "%s: cache_slots=%lld out of range (0, 2^31)", who,
              (long long)cache_slots);
  if (batch == 0) return NVL_OK;
  // more than 64 KiB of LDS is an opt-in, made once per device for the full table: the first call must come before any
  // graph capture (hipFuncSetAttribute is not a stream operation; the engine makes that call at start-up)
  constexpr size_t full = (size_t)kPenFields * 2 + kPenSpare;
  static bool attr_done[NVL_MAX_DEVICES] = {};
  bool& attr_set = attr_done[nvl_device_slot()];
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&penalty_apply_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)full) != hipSuccess) {
      nvl_set_error("%s: cannot reserve %zu B of LDS", who, full);
      return NVL_ELAUNCH;
    }
    attr_set = true;
  }
  int bs_shift = 0;
  while ((1 << bs_shift) < block_size) ++bs_shift;
  const int64_t fields = vocab < kPenFields ? vocab : kPenFields;
  const size_t lds = (size_t)((fields + 7) / 8) * 16 + kPenSpare;
  hipLaunchKernelGGL(penalty_apply_kernel, dim3((unsigned)batch, (unsigned)((vocab + kPenFields - 1) / kPenFields)), dim3(kPenThreads), lds, (hipStream_t)stream,
                     (bf16_t*)logits, logits_row_stride, token_cache, cache_slots, block_tables, bt_stride, max_blocks,
                     context_lens, prompt_lens, presence, frequency, repetition, (int)vocab, bs_shift, (int)max_context);
  return nvl_check_launch(who);
}
