// The state into the data sections of Fortran FV3 restart files (NetCDF-3: dense, BIG-endian), with the sums FMS stamps every
// variable with: the inverse of the XFAST path of k_state_unpack.  Up to PACE_RESTART_MAX_ITEMS windows of fields are gathered by
// ONE launch into one device byte buffer, and the wrapping 64-bit sum of every item's bit patterns comes out of the same pass.
//
// Fields are stored [k][j][i], i fastest, rows padded (IDX3).  An item's output element is e = i + ni * (j + nj * k): the file's
// (z, y, x) C order is the storage's own order -- nothing is transposed, the row padding is dropped.  The value is the field's
// element widened to double (exact), for PACE_RESTART_BE_F32 narrowed by a plain cast, byte-swapped and stored.
//
//   k_restart_pack     1-D grid, 256 threads = 4 waves.  The output is dense, so the launch is indexed by OUTPUT element.  An
//                      item's elements are cut into 16-byte SLOTS of the output (V = 2 doubles or 4 floats) counted from the
//                      16-byte boundary at or below its first byte: with `shift` = the elements between that boundary and the
//                      item's first one (0 .. V - 1; offsets are only element-aligned), slot s holds elements V * s - shift ..
//                      V * s - shift + V - 1.  A slot that lies wholly inside the item is ONE 16-byte store at an aligned
//                      address; the first slot (head) and the last (tail) may hold fewer elements and store them one by one.
//                      A workgroup takes RS_SLOTS = 4 * 256 consecutive slots (16 KiB of output), thread t the slots t,
//                      t + 256, ...: a wave's store is 1 KiB contiguous.  It finds its item by table_find (wgmap.h) in the
//                      table that travels by value (pack_table.h).
//           loads      per element, no LDS stage.  The window's rows are 12 .. 391 elements and start at any element, so no
//                      vector load is aligned; but consecutive output elements ARE consecutive addresses within a row, and a
//                      wave's V load instructions together read the same 128 (256) consecutive elements -- whole cache lines but
//                      for the row ends, each line fetched from L2 once (the second instruction finds it in the vector L1).  An
//                      LDS stage (coalesced loads of element l, l + 64; pairs read back) would turn the V strided loads into V
//                      contiguous ones and add a barrier and two LDS passes: nothing is transposed here, so unlike k_diag_pack's
//                      tile there is no access it would make contiguous that is not already.  (e -> i, j, k costs two 32-bit
//                      divisions per slot; the elements of a slot then step i with a carry.)
//           sums       one 64-bit accumulator per thread, integer addition: shuffles over the 64 lanes, LDS over the 4 waves,
//                      thread 0 writes the workgroup's partial -- EVERY workgroup writes one, so the workspace needs no clearing
//                      and holds nothing between calls.
//   k_restart_combine  grid (nitems), one wave: lane l folds the item's partials l, l + 64, ..., then the same shuffles.
//
// No atomics, no host synchronisation: integer addition wraps and commutes, so the sums do not depend on the order workgroups
// run in.  Nothing outside a window is read (not the halo, not other levels, not the row padding); nothing outside an item's
// ni * nj * nk elements is written.  float64 storage -> BE_F64 moves bits: -0.0, denormals, +-inf and NaN payloads arrive
// unchanged (the value never passes through a floating-point instruction).
#include "common.h"
#include "kernels.h"
#include "pack_table.h"

#define RS_WAVES 4
#define RS_UNROLL 4
#define RS_SLOTS (64 * RS_WAVES * RS_UNROLL)  // 16-byte slots of the output per workgroup

struct RestartEntry {
  const real* field;
  int i0, j0, k0, ni, nj, kind;
  int total;      // ni * nj * nk output elements
  int shift;      // elements between the 16-byte boundary below the item's first output byte and that byte
  long out_byte;  // of the item's first element
};

typedef PackTable<RestartEntry, PACE_RESTART_MAX_ITEMS> RestartTable;

struct alignas(16) RestartSlot {
  uint64_t w[2];
};

// the bit pattern of the value as the file holds it, before the swap
template <typename OutT>
__device__ __forceinline__ uint64_t restart_bits(real v);
template <>
__device__ __forceinline__ uint64_t restart_bits<double>(real v) {
  uint64_t b;
  if (sizeof(real) == 8) {
    memcpy(&b, &v, 8);  // a move of bits
  } else {
    const double d = (double)v;
    memcpy(&b, &d, 8);
  }
  return b;
}
template <>
__device__ __forceinline__ uint64_t restart_bits<float>(real v) {
  const float f = (float)(double)v;
  uint32_t b;
  memcpy(&b, &f, 4);
  return (uint64_t)b;
}

// every lane of the wave must call it; lane 0 ends with the wave's sum
__device__ __forceinline__ uint64_t restart_wave_sum(uint64_t s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += (uint64_t)__shfl_down((unsigned long long)s, (unsigned)d, 64);
  return s;
}

template <typename OutT>
__global__ void __launch_bounds__(64 * RS_WAVES) k_restart_pack(Geo g, RestartTable tab, unsigned char* __restrict__ out,
                                                                 uint64_t* __restrict__ partial) {
  constexpr int V = 16 / (int)sizeof(OutT);
  const int b = (int)blockIdx.x;
  const int m = table_find(tab.first, tab.nitems, b);
  const RestartEntry& it = tab.item[m];
  const real* __restrict__ q = it.field;
  const int ni = it.ni, nj = it.nj, total = it.total, shift = it.shift;
  const bool vol = it.kind == PACE_DIAG_WINDOW3D;
  // the item's first element is at out_byte; slot 0 starts `shift` elements below it, on a 16-byte boundary
  OutT* __restrict__ o = out ? (OutT*)(out + it.out_byte) : nullptr;
  const int slot0 = (b - tab.first[m]) * RS_SLOTS + (int)threadIdx.x;

  uint64_t sum = 0;
#pragma unroll
  for (int u = 0; u < RS_UNROLL; ++u) {
    const int e0 = (slot0 + u * 64 * RS_WAVES) * V - shift;  // the slot's first element: >= -shift
    if (e0 >= total) break;
    const int ef = e0 < 0 ? 0 : e0;
    const int r = ef / ni;
    int i = ef - r * ni, k = r / nj;
    int j = r - k * nj;
    uint64_t w[V];
#pragma unroll
    for (int t = 0; t < V; ++t) {
      const int e = e0 + t;
      w[t] = 0;
      if (e >= 0 && e < total) {
        const real v = vol ? q[IDX3(g, it.i0 + i, it.j0 + j, it.k0 + k)] : q[IDX2(g, it.i0 + i, it.j0 + j)];
        w[t] = restart_bits<OutT>(v);
        sum += w[t];
        if (++i == ni) {
          i = 0;
          if (++j == nj) {
            j = 0;
            ++k;
          }
        }
      }
    }
    if (o == nullptr) continue;
    if (e0 >= 0 && e0 + V <= total) {
      RestartSlot s;
      if (V == 2) {
        s.w[0] = __builtin_bswap64(w[0]);
        s.w[1] = __builtin_bswap64(w[1]);
      } else {  // little-endian words: the element at the lower address in the low half
        s.w[0] = (uint64_t)__builtin_bswap32((uint32_t)w[0]) | ((uint64_t)__builtin_bswap32((uint32_t)w[1 % V]) << 32);
        s.w[1] = (uint64_t)__builtin_bswap32((uint32_t)w[2 % V]) | ((uint64_t)__builtin_bswap32((uint32_t)w[3 % V]) << 32);
      }
      *(RestartSlot*)(o + e0) = s;
    } else {
#pragma unroll
      for (int t = 0; t < V; ++t) {
        const int e = e0 + t;
        if (e < 0 || e >= total) continue;
        if (V == 2) {
          const uint64_t x = __builtin_bswap64(w[t]);
          memcpy(o + e, &x, sizeof(OutT));
        } else {
          const uint32_t x = __builtin_bswap32((uint32_t)w[t]);
          memcpy(o + e, &x, sizeof(OutT));
        }
      }
    }
  }

  if (partial == nullptr) return;  // (uniform over the launch)
  sum = restart_wave_sum(sum);
  __shared__ uint64_t per_wave[RS_WAVES];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (lane == 0) per_wave[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < RS_WAVES; ++v) sum += per_wave[v];
    partial[b] = sum;
  }
}

__global__ void __launch_bounds__(64) k_restart_combine(RestartTable tab, const uint64_t* __restrict__ partial,
                                                        uint64_t* __restrict__ sums) {
  const int m = (int)blockIdx.x;
  uint64_t s = 0;
  for (int b = tab.first[m] + (int)threadIdx.x; b < tab.first[m + 1]; b += 64) s += partial[b];
  s = restart_wave_sum(s);
  if (threadIdx.x == 0) sums[m] = s;
}

// workgroups of an item: its slots, counted from the 16-byte boundary below its first byte (shift <= V - 1)
static inline long restart_blocks(long total, int shift, int v) {
  const long slots = (total + shift + v - 1) / v;
  return (slots + RS_SLOTS - 1) / RS_SLOTS;
}

// an upper bound that does not depend on out or out_type: the float64 slots (2 elements) with the largest shift
size_t restart_pack_workspace_bytes(const pace_restart_item_t* items, int nitems) {
  long blocks = 0;
  for (int m = 0; m < nitems; ++m) blocks += restart_blocks((long)items[m].ni * items[m].nj * items[m].nk, 1, 2);
  return (size_t)blocks * sizeof(uint64_t);
}

int launch_restart_pack(const Geo& g, const pace_restart_item_t* items, int nitems, int out_type, void* out, uint64_t* sums,
                        void* workspace, hipStream_t st) {
  const int esize = out_type == PACE_RESTART_BE_F64 ? 8 : 4, v = 16 / esize;
  RestartTable tab{};
  tab.nitems = nitems;
  for (int m = 0; m < nitems; ++m) {
    const pace_restart_item_t& in = items[m];
    RestartEntry& e = tab.item[m];
    e.field = in.field;
    e.i0 = in.i0, e.j0 = in.j0, e.k0 = in.k0, e.ni = in.ni, e.nj = in.nj, e.kind = in.kind;
    e.total = in.ni * in.nj * in.nk;  // (within the storage: below 2^29, geom_check)
    e.out_byte = in.out_offset;
    e.shift = out ? (int)(((uintptr_t)out + (uintptr_t)in.out_offset) % 16) / esize : 0;
  }
  const int rc = pack_table_fill_first(tab, [v](const RestartEntry& e) { return restart_blocks(e.total, e.shift, v); });
  if (rc != PACE_OK) return rc;
  const dim3 grid((unsigned)tab.first[nitems]), block(64 * RS_WAVES);
  uint64_t* partial = sums ? (uint64_t*)workspace : nullptr;
  if (out_type == PACE_RESTART_BE_F64)
    hipLaunchKernelGGL(k_restart_pack<double>, grid, block, 0, st, g, tab, (unsigned char*)out, partial);
  else
    hipLaunchKernelGGL(k_restart_pack<float>, grid, block, 0, st, g, tab, (unsigned char*)out, partial);
  PACE_CHECK_LAUNCH();
  if (sums) {
    hipLaunchKernelGGL(k_restart_combine, dim3((unsigned)nitems), dim3(64), 0, st, tab, (const uint64_t*)partial, sums);
    PACE_CHECK_LAUNCH();
  }
  return PACE_OK;
}
