// gsd_block_prims.h -- the wave and block building blocks of the geometry kernels: __device__ templates
// only, no kernel.  A wave is 64 lanes, a block THREADS = 64 * waves threads, every thread of the block makes every call.
#pragma once
#include <hip/hip_runtime.h>

// ---- wave: the xor butterfly (lane l meets l ^ 32, then l ^ 16, ... l ^ 1; every lane gets the result) ---------------------
template <typename T>
__device__ __forceinline__ T gsd_wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <typename T>
__device__ __forceinline__ T gsd_wave_max(T v) {      // a NaN never replaces a number
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T gsd_wave_min(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}
// lane l gets v of the lanes 0..l
template <typename T>
__device__ __forceinline__ T gsd_wave_inclusive_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// ---- block ------------------------------------------------------------------------------------------------------------------
// The sum of every wave's `wave_n` (the same value in all lanes of a wave), returned to thread 0 alone.  lds: THREADS / 64 ints.
template <int THREADS>
__device__ __forceinline__ int gsd_block_count(int wave_n, int* lds) {
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = wave_n;
  __syncthreads();
  int n = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) n += lds[w];
  }
  return n;
}

// The totals of the waves in front of the caller's, from every thread's gsd_wave_inclusive_scan value (lane 63 holds its wave's
// total): with `inclusive` - own, a weighted rank in the block.  lds: THREADS / 64 ints.
template <int THREADS>
__device__ __forceinline__ int gsd_block_waves_before(int inclusive, int* lds) {
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) lds[wave] = inclusive;
  __syncthreads();
  int before = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) before += w < wave ? lds[w] : 0;
  return before;
}

// A block works on ROUNDS * THREADS items, thread t on item j * THREADS + t in round j; mask[j] is the wave's __ballot of "my item
// of round j counts".  rank[j] becomes the number of counting items in front of the thread's own in item order: the (round, wave)
// slots in front of its slot + the lanes below it.  lds: ROUNDS * THREADS / 64 ints.
template <int THREADS, int ROUNDS>
__device__ __forceinline__ void gsd_block_rank(const unsigned long long (&mask)[ROUNDS], int* lds, int (&rank)[ROUNDS]) {
  constexpr int WAVES = THREADS / 64, SLOTS = ROUNDS * WAVES;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) lds[j * WAVES + wave] = __popcll(mask[j]);
  }
  __syncthreads();
  int n[SLOTS];
#pragma unroll
  for (int v = 0; v < SLOTS; ++v) n[v] = lds[v];
#pragma unroll
  for (int j = 0; j < ROUNDS; ++j) {
    int before = 0;
#pragma unroll
    for (int v = 0; v < SLOTS; ++v) before += v < j * WAVES + wave ? n[v] : 0;
    rank[j] = before + __popcll(mask[j] & ((1ull << lane) - 1ull));
  }
}

// One block's exclusive scan of n counts, THREADS * PER of them per pass with a carry from pass to pass, so any n is served.
// Thread t of a pass takes the PER consecutive items from base + t * PER on: load(i) yields count i, store(i, x) receives the sum
// of the counts in front of it; all loads of a pass come before its stores, so the two may name the same memory.  The sums are
// kept in Acc (int or long long).  Returns the total to every thread; the stores are visible to the block by then.
template <typename Acc, int THREADS, int PER, typename Load, typename Store>
__device__ __forceinline__ Acc gsd_block_exclusive_scan(int n, Load load, Store store) {
  __shared__ Acc wave_total[THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Acc carry = 0;
  for (int base = 0; base < n; base += THREADS * PER) {      // n + THREADS * PER stays below 2^31: the callers' hosts see to it
    const int i0 = base + tid * PER;
    Acc v[PER];
    Acc s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      v[j] = i0 + j < n ? (Acc)load(i0 + j) : (Acc)0;
      s += v[j];
    }
    const Acc inc = gsd_wave_inclusive_scan(s);
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    Acc before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
      const Acc x = wave_total[w];
      before += w < wave ? x : 0;
      all += x;
    }
    Acc run = carry + before + inc - s;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (i0 + j < n) store(i0 + j, run);
      run += v[j];
    }
    carry += all;
    __syncthreads();      // wave_total is reused; the stores are visible to the block
  }
  return carry;
}
