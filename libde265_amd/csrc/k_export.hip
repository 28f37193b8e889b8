// k_export.hip -- the export of a decoded picture into caller-owned device buffers (de265hip_dpb_export_async).
//
// One launch per picture covers all its output planes.  The grid is sized to the device (host.hip) and strides over the rows
// of all planes, a workgroup at a time per row; its threads take 16-byte chunks of the OUTPUT row.  A streaming kernel: what
// matters is full-width accesses and enough of them in flight, so every chunk is one 16-byte store and (where the source
// allows it) one load of the source bytes it needs.
//
// Output definition (include/de265_hip.h, "export"; restated in numpy by tests/test_export_abi.py):
//   window   the host offsets src by the crop in SAMPLES at every bit depth (libde265's pixels_confwin offsets a byte pointer by
//            samples, image.cc:385-387, which differs for left / top crops of pictures of more than 8 bits)
//   layout   planar: one source per output plane; semi-planar CbCr: output element e is sample e/2 of Cb (e even) or Cr (e odd)
//   format   NATIVE v (uint8 at 8 bit, else uint16) | MSB16 v << (16 - bd) | F32 (float)v / (float)((1 << bd) - 1), correctly
//            rounded (no fast-math: HIP's fp32 division is IEEE) | F16 that float rounded to nearest-even
//
// Chunks: a row's first `head` elements reach the first 16-byte boundary of the destination row (its base and pitch need not be
// aligned: torch views with storage offsets, odd pitches); every later full chunk of 16 bytes is one vector store, its source one
// vector load when that is aligned too (a left crop may shift it), element loads otherwise; the rest (head, tail, a semi-planar
// row whose boundary falls inside a CbCr pair) goes element by element.
#include "export.h"
#include "../../include/de265_hip.h"

namespace d265 {

namespace {

template <typename S, int FMT> struct OutOf { using T = S; };                 // NATIVE: the source type
template <typename S> struct OutOf<S, DE265HIP_EXPORT_MSB16> { using T = uint16_t; };
template <typename S> struct OutOf<S, DE265HIP_EXPORT_F32> { using T = float; };
template <typename S> struct OutOf<S, DE265HIP_EXPORT_F16> { using T = uint16_t; };   // (the half's bits)

template <int B> struct VecOf;
template <> struct VecOf<16> { using T = uint4; };
template <> struct VecOf<8> { using T = uint2; };
template <> struct VecOf<4> { using T = uint32_t; };
template <> struct VecOf<2> { using T = uint16_t; };

// N consecutive samples from p: one load of N * sizeof(S) bytes when p is aligned to it, element loads otherwise
template <typename S, int N>
__device__ __forceinline__ void load_n(const S* p, S (&v)[N])
{
  constexpr int B = N * (int)sizeof(S);
  if (((uintptr_t)p & (B - 1)) == 0) {
    const typename VecOf<B>::T x = *reinterpret_cast<const typename VecOf<B>::T*>(p);
    __builtin_memcpy(v, &x, B);
  } else {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = p[i];
  }
}

template <typename S, int FMT>
__device__ __forceinline__ typename OutOf<S, FMT>::T conv(uint32_t v, int bd, float den)
{
  if constexpr (FMT == DE265HIP_EXPORT_NATIVE) return (S)v;
  else if constexpr (FMT == DE265HIP_EXPORT_MSB16) return (uint16_t)(v << (16 - bd));
  else if constexpr (FMT == DE265HIP_EXPORT_F32) return (float)v / den;
  else { const _Float16 h = (_Float16)((float)v / den); return __builtin_bit_cast(uint16_t, h); }
}

template <typename S, int FMT>
__device__ __forceinline__ void export_row(const ExportPlane& P, int r)
{
  using O = typename OutOf<S, FMT>::T;
  constexpr int K = 16 / (int)sizeof(O);
  const int bd = P.bd;
  const float den = (float)((1 << bd) - 1);
  const S* s0 = reinterpret_cast<const S*>(P.src[0] + (int64_t)r * P.spitch);
  const S* s1 = P.semi ? reinterpret_cast<const S*>(P.src[1] + (int64_t)r * P.spitch) : s0;
  O* d = reinterpret_cast<O*>(P.dst + (int64_t)r * P.dpitch);       // (aligned to the element size: checked by the host)
  const int cols = P.cols;
  int head = (int)(((16u - ((uint32_t)(uintptr_t)d & 15u)) & 15u) / sizeof(O));
  const bool vec = !(P.semi && (head & 1));                          // (a CbCr pair across the boundary: the whole row by elements)
  if (!vec) head = 0;
  head = min(head, cols);
  const int nch = 1 + (cols - head + K - 1) / K;
  for (int j = threadIdx.x; j < nch; j += blockDim.x) {
    const int e0 = j ? head + (j - 1) * K : 0, e1 = j ? min(e0 + K, cols) : head;
    if (vec && j && e1 - e0 == K) {
      O o[K];
      if (!P.semi) {
        S v[K];
        load_n<S, K>(s0 + e0, v);
#pragma unroll
        for (int i = 0; i < K; i++) o[i] = conv<S, FMT>(v[i], bd, den);
      } else {
        S a[K / 2], b[K / 2];
        load_n<S, K / 2>(s0 + (e0 >> 1), a);
        load_n<S, K / 2>(s1 + (e0 >> 1), b);
#pragma unroll
        for (int i = 0; i < K / 2; i++) { o[2 * i] = conv<S, FMT>(a[i], bd, den); o[2 * i + 1] = conv<S, FMT>(b[i], bd, den); }
      }
      uint4 u;
      __builtin_memcpy(&u, o, 16);
      *reinterpret_cast<uint4*>(d + e0) = u;
    } else {
      for (int e = e0; e < e1; e++) {
        const uint32_t v = P.semi ? ((e & 1) ? s1 : s0)[e >> 1] : s0[e];
        d[e] = conv<S, FMT>(v, bd, den);
      }
    }
  }
}

template <typename S, int FMT>
__global__ __launch_bounds__(256) void k_export(ExportJob J)
{
  for (int fr = blockIdx.x; fr < J.total_rows; fr += gridDim.x) {
    if (J.n_planes > 2 && fr >= J.p[2].row_start) export_row<S, FMT>(J.p[2], fr - J.p[2].row_start);
    else if (J.n_planes > 1 && fr >= J.p[1].row_start) export_row<S, FMT>(J.p[1], fr - J.p[1].row_start);
    else export_row<S, FMT>(J.p[0], fr);
  }
}

template <typename S>
hipError_t launch_fmt(const ExportJob& J, hipStream_t st, int grid)
{
  switch (J.format) {
  case DE265HIP_EXPORT_NATIVE: hipLaunchKernelGGL((k_export<S, DE265HIP_EXPORT_NATIVE>), dim3(grid), dim3(256), 0, st, J); break;
  case DE265HIP_EXPORT_MSB16: hipLaunchKernelGGL((k_export<S, DE265HIP_EXPORT_MSB16>), dim3(grid), dim3(256), 0, st, J); break;
  case DE265HIP_EXPORT_F32: hipLaunchKernelGGL((k_export<S, DE265HIP_EXPORT_F32>), dim3(grid), dim3(256), 0, st, J); break;
  case DE265HIP_EXPORT_F16: hipLaunchKernelGGL((k_export<S, DE265HIP_EXPORT_F16>), dim3(grid), dim3(256), 0, st, J); break;
  default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_export(const ExportJob& J, hipStream_t st, int grid)
{
  return J.src16 ? launch_fmt<uint16_t>(J, st, grid) : launch_fmt<uint8_t>(J, st, grid);
}

}  // namespace d265
