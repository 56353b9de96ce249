// Layout rules of the 1-bit sign store (PH_ROWS_BITS), shared by the library (rowstore.hip, phnsw_device.h) and the
// stand-alone host test (tests/cpp/test_bits_plan.cpp).  Plain C++: no HIP header is needed to include this file.
//
//   bit j of a row       = ph_bits_sign(rows[i][j]): the component is below zero (+0, -0, every non-negative value: 0)
//   public layout        = [n][ph_bits_words(dim)] words, component j in bit j & 31 of word j >> 5 (phnsw_bits_read)
//   device layout        = rows of ph_bits_stride(nv) = 32 * nv bytes, nv = ph_bits_class(dim) = 1 / 3 / 6 for up to
//                          256 / 768 / 1536 components: the same words in the same order, then zero words
//   padding              = every bit j >= dim of a device row, and of a query reduced to bits, is 0
//   h                    = popcount(row XOR query) over the device row's words
//   distance             = dot metrics: r = dim - 2 h;  Euclidean: r = 4 h;  then the metric's own last step
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PH_BITS_HD __host__ __device__
#else
#define PH_BITS_HD
#endif

#define PH_BITS_MAX_DIM 1536u

// the sign rule, written on the bits of the float so that it does not depend on a denormal mode: negative, not a zero,
// not a NaN
PH_BITS_HD static inline uint32_t ph_bits_sign_of(uint32_t u) {
  const uint32_t mag = u & 0x7FFFFFFFu;
  return ((u >> 31) != 0u && mag != 0u && mag <= 0x7F800000u) ? 1u : 0u;
}
static inline uint32_t ph_bits_sign(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return ph_bits_sign_of(u);
}
PH_BITS_HD static inline uint32_t ph_bits_ld(uint32_t dim) { return (dim + 3u) & ~3u; }       // components of a padded f32 row
PH_BITS_HD static inline uint32_t ph_bits_words(uint32_t dim) { return (dim + 31u) / 32u; }  // public words per row
// chunk class of a dimension (ph_chunk_count of the padded row's float4 count): 0 = unsupported
PH_BITS_HD static inline int ph_bits_class(uint32_t dim) {
  const uint32_t nv4 = ph_bits_ld(dim) / 4u;
  return dim == 0u ? 0 : (nv4 <= 64u ? 1 : (nv4 <= 192u ? 3 : (nv4 <= 384u ? 6 : 0)));
}
PH_BITS_HD static inline uint32_t ph_bits_stride(int nv) { return 32u * (uint32_t)nv; }       // bytes per device row
PH_BITS_HD static inline uint32_t ph_bits_stride_words(int nv) { return 8u * (uint32_t)nv; }  // words per device row
PH_BITS_HD static inline uint32_t ph_bits_word_of(uint32_t j) { return j >> 5; }
PH_BITS_HD static inline uint32_t ph_bits_bit_of(uint32_t j) { return j & 31u; }
// word index of component j of row i in the device allocation (in words)
PH_BITS_HD static inline uint64_t ph_bits_device_word(uint64_t i, uint32_t j, int nv) {
  return i * (uint64_t)ph_bits_stride_words(nv) + ph_bits_word_of(j);
}
// the value before the metric's last step, from the Hamming distance h of two sign vectors of `dim` components
PH_BITS_HD static inline float ph_bits_raw(uint32_t h, uint32_t dim, bool l2) {
  return l2 ? (float)(4u * h) : (float)((int)dim - 2 * (int)h);
}
