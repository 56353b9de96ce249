// The layout rules of the bits row store (parallel_hnsw_amd/csrc/bits_plan.h) over every dimension 1 .. 1536, with a host
// model of the conversion kernel and of the distance's row indexing over arrays of exactly the sizes the launchers
// allocate: an index past a row, a padding bit that is set, a word the conversion leaves unwritten or a stride that
// breaks the 16-byte alignment stops the program (AddressSanitizer / UBSan: tests/test_bits_plan_cpp.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/bits_plan.h"

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      printf("FAILED %s:%d: %s (dim %u)\n", __FILE__, __LINE__, #c, g_dim); \
      exit(1);                                                       \
    }                                                                \
  } while (0)
static uint32_t g_dim = 0;

static uint32_t popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// ph_bits_convert_kernel as the host runs it: 64 components at a time, one ballot = two words, lane w keeps word w, the
// row's stride_words words leave in one store
static void convert_row(const float *src, uint32_t dim, uint32_t *dst, uint32_t stride_words) {
  uint32_t word[64] = {0};
  for (uint32_t b = 0; 64u * b < dim; b++) {
    uint64_t m = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint32_t c = 64u * b + lane;
      if (c < dim && ph_bits_sign(src[c])) m |= 1ull << lane;
    }
    CHECK(2u * b + 1u < 64u);
    word[2u * b] = (uint32_t)m;
    word[2u * b + 1u] = (uint32_t)(m >> 32);
  }
  for (uint32_t lane = 0; lane < 64; lane++)
    if (lane < stride_words) dst[lane] = word[lane];
}

int main() {
  // the sign rule on the edges of f32
  CHECK(ph_bits_sign(0.0f) == 0 && ph_bits_sign(-0.0f) == 0 && ph_bits_sign(1.0f) == 0);
  CHECK(ph_bits_sign(-1.0f) == 1 && ph_bits_sign(-1.4e-45f) == 1 && ph_bits_sign(1.4e-45f) == 0);
  CHECK(ph_bits_sign(-INFINITY) == 1 && ph_bits_sign(INFINITY) == 0 && ph_bits_sign(-NAN) == 0 && ph_bits_sign(NAN) == 0);
  const uint64_t n = 5;  // rows of the model store: the first, the last and three between
  for (uint32_t dim = 1; dim <= PH_BITS_MAX_DIM; dim++) {
    g_dim = dim;
    const int nv = ph_bits_class(dim);
    CHECK(nv == 1 || nv == 3 || nv == 6);
    const uint32_t ld = ph_bits_ld(dim), sw = ph_bits_stride_words(nv), words = ph_bits_words(dim);
    CHECK(ld >= dim && ld % 4 == 0 && ld < dim + 4);
    CHECK(ph_bits_stride(nv) == 4u * sw && ph_bits_stride(nv) % 16u == 0);  // rows start on 16-byte boundaries
    CHECK(256u * (uint32_t)nv >= ld && words <= sw && sw <= 48u);          // a row holds every component; a wave stores it at once
    CHECK((nv == 1) == (dim <= 256) && (nv == 3) == (dim > 256 && dim <= 768));
    CHECK(ph_bits_word_of(dim - 1) == words - 1 && ph_bits_bit_of(dim - 1) == ((dim - 1) & 31u));
    // rows as the f32 store holds them ([n][ld], padding zero) and the device allocation, exactly n * stride bytes
    std::vector<float> rows(n * ld, 0.0f);
    for (uint64_t i = 0; i < n; i++)
      for (uint32_t j = 0; j < dim; j++) {
        const uint32_t r = (uint32_t)((i * 2654435761u + j * 40503u + dim) >> 3);
        rows[i * ld + j] = (r % 3u == 0) ? -1.0f - (float)(r % 7u) : ((r % 3u == 1) ? (float)(r % 5u) : -0.0f);
      }
    for (uint32_t j = 0; j < dim; j++) rows[4 * ld + j] = -2.0f;  // the last row: every bit
    std::vector<uint32_t> dev(n * sw, 0xDEADBEEFu);
    for (uint64_t i = 0; i < n; i++) convert_row(&rows[i * ld], dim, &dev[i * sw], sw);
    for (uint64_t i = 0; i < n; i++) {
      uint32_t set = 0;
      for (uint32_t j = 0; j < dim; j++) {
        const uint64_t w = ph_bits_device_word(i, j, nv);
        CHECK(w < n * sw && w / sw == i);  // a component's word lies inside its own row
        const uint32_t bit = (dev[w] >> ph_bits_bit_of(j)) & 1u;
        CHECK(bit == ph_bits_sign(rows[i * ld + j]));
        set += bit;
      }
      uint32_t all = 0;
      for (uint32_t w = 0; w < sw; w++) all += popc(dev[i * sw + w]);
      CHECK(all == set);  // every padding bit is 0, every word of the row was written
      if (i == 4) CHECK(set == dim);
    }
    // the public layout: the leading ceil(dim / 32) words of a device row (phnsw_bits_read copies exactly those)
    CHECK((uint64_t)(n - 1) * sw + words <= n * sw);
    // the distance: 2 nv 16-byte loads per row = the whole row and nothing past it; h against a model on the floats
    CHECK(2u * (uint32_t)nv * 4u == sw);
    for (uint64_t a = 0; a < n; a++) {
      const uint64_t b = (a + 1) % n;
      uint32_t h = 0, want = 0;
      for (uint32_t i = 0; i < 2u * (uint32_t)nv; i++)
        for (uint32_t e = 0; e < 4; e++) {
          const uint64_t wa = a * sw + 4u * i + e, wb = b * sw + 4u * i + e;
          CHECK(wa < n * sw && wb < n * sw);
          h += popc(dev[wa] ^ dev[wb]);
        }
      for (uint32_t j = 0; j < dim; j++) want += ph_bits_sign(rows[a * ld + j]) != ph_bits_sign(rows[b * ld + j]);
      CHECK(h == want && h <= dim);
      // the values before the metric's last step are the f32 sums over the +-1 rows, exactly
      float dot = 0.f, l2 = 0.f;
      for (uint32_t j = 0; j < dim; j++) {
        const float x = ph_bits_sign(rows[a * ld + j]) ? -1.f : 1.f, y = ph_bits_sign(rows[b * ld + j]) ? -1.f : 1.f;
        dot += x * y;
        l2 += (x - y) * (x - y);
      }
      CHECK(ph_bits_raw(h, dim, false) == dot && ph_bits_raw(h, dim, true) == l2);
    }
  }
  g_dim = 0;
  CHECK(ph_bits_class(0) == 0 && ph_bits_class(1537) == 0 && ph_bits_class(1536) == 6);
  printf("ALL OK\n");
  return 0;
}
