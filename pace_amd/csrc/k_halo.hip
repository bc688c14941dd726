// Halo-exchange pack / unpack (replaces HaloDataTransformerGPU's pack/unpack kernels and the rotate + slice logic
// in front of them: util/pace/util/halo_data_transformer.py:150-921, rotate.py:4-50, _boundary_utils.py:58-95).
//
// A message strip is addressed in the RECEIVER's orientation: element (a, b, k) lands at field index
// (ri0 + a, rj0 + b, k) on the receiving tile.  The sender reads it from (i0 + a*di_a + b*di_b,
// j0 + a*dj_a + b*dj_b, k) -- the tile-to-tile rotation, the component swap of vector fields and their sign are all
// folded into that affine map and `sign` by the host (pace_amd/util/halo.py), so packing IS the rotation and the
// receiver only copies.  One launch moves every strip of every field of an updater (blockIdx.y = strip).
// Message layout [k][b][a]: rows of `a` (the receiver's i) are contiguous.  HBM/latency-bound, tiny.
#include "common.h"
#include "kernels.h"

#define HALO_MAX_DESC 16
struct HaloBatch {
  pace_halo_desc_t d[HALO_MAX_DESC];
};

template <int UNPACK>
__global__ void __launch_bounds__(256) k_halo_copy(Geo g, HaloBatch batch) {
  const pace_halo_desc_t& d = batch.d[blockIdx.y];
  const long total = (long)d.na * d.nb * d.nk;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int a = (int)(e % d.na);
    const long r = e / d.na;
    const int b = (int)(r % d.nb);
    const int k = (int)(r / d.nb);
    const long f = IDX3(g, d.i0 + a * d.di_a + b * d.di_b, d.j0 + a * d.dj_a + b * d.dj_b, k);
    if (UNPACK) d.field[f] = d.buf[e];
    else d.buf[e] = d.sign * d.field[f];
  }
}

int launch_halo_copy(const Geo& g, const pace_halo_desc_t* descs, int ndesc, int unpack, hipStream_t st) {
  for (int base = 0; base < ndesc; base += HALO_MAX_DESC) {
    const int n = (ndesc - base < HALO_MAX_DESC) ? ndesc - base : HALO_MAX_DESC;
    HaloBatch batch;
    long most = 1;
    for (int t = 0; t < n; ++t) {
      batch.d[t] = descs[base + t];
      const long tot = (long)descs[base + t].na * descs[base + t].nb * descs[base + t].nk;
      if (tot > most) most = tot;
    }
    for (int t = n; t < HALO_MAX_DESC; ++t) batch.d[t] = batch.d[0];
    long bx = (most + 255) / 256;
    if (bx > 1024) bx = 1024;
    const dim3 grid((unsigned)bx, (unsigned)n), block(256);
    if (unpack) hipLaunchKernelGGL(k_halo_copy<1>, grid, block, 0, st, g, batch);
    else hipLaunchKernelGGL(k_halo_copy<0>, grid, block, 0, st, g, batch);
  }
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

// The halo update of tiles that share a device (pace_halo_cube): no message, no staging buffer -- a workgroup row reads the
// sender's field through the strip's affine map and writes the receiver's halo.  One launch for every strip of every field of
// every tile: blockIdx.y = entry of the table, blockIdx.x = chunk of the strip.  The table lies in device memory (hundreds of
// entries: no by-value batch holds them); an entry is the same for the whole workgroup, so it is fetched by scalar loads (the
// pointer is const __restrict__: nothing the kernel writes can alias it) and costs the lanes nothing.
// Strips are 1..3 points across: the host names the direction of the longer unit-stride run (on either side) and consecutive
// lanes walk it (PACE_HALO_XFER_B_FAST), so a wave touches runs of whole rows instead of 64 different ones.
__global__ void __launch_bounds__(256) k_halo_cube(Geo g, const pace_halo_xfer_t* __restrict__ table) {
  const pace_halo_xfer_t d = table[blockIdx.y];
  const unsigned total = (unsigned)d.na * (unsigned)d.nb * (unsigned)d.nk;
  const bool b_fast = (d.flags & PACE_HALO_XFER_B_FAST) != 0;
  const unsigned nf = (unsigned)(b_fast ? d.nb : d.na), ns = (unsigned)(b_fast ? d.na : d.nb);
  for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
    const unsigned r = e / nf;
    const int f = (int)(e - r * nf), k = (int)(r / ns), s = (int)(r - (unsigned)k * ns);
    const int a = b_fast ? s : f, b = b_fast ? f : s;
    const real v = d.src[IDX3(g, d.i0 + a * d.di_a + b * d.di_b, d.j0 + a * d.dj_a + b * d.dj_b, k)];
    d.dst[IDX3(g, d.ri0 + a, d.rj0 + b, k)] = (real)(d.sign * v);
  }
}

int launch_halo_cube(const Geo& g, const pace_halo_xfer_t* table_on_device, int n, hipStream_t st) {
  // the largest strip a field of this geometry can hold bounds the 32-bit element counter of the kernel
  const long most = (long)g.ni * g.nj * (g.nk + 1);
  if (most >= (1L << 31)) return PACE_ERR_UNSUPPORTED;
  // chunks for a three-point strip along a whole edge; longer strips take more turns of the kernel's loop
  long bx = (3L * (g.n + 1) * (g.nk + 1) + 255) / 256;
  if (bx > 1024) bx = 1024;
  for (int base = 0; base < n; base += 65535) {  // (gridDim.y)
    const int rows = n - base < 65535 ? n - base : 65535;
    hipLaunchKernelGGL(k_halo_cube, dim3((unsigned)bx, (unsigned)rows), dim3(256), 0, st, g, table_on_device + base);
  }
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
