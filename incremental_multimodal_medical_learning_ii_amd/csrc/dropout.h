// Counter-based dropout masks for the CXR-BERT encoder (HF BertModel's four dropout sites, train mode).
//
// Every keep decision is a pure function of (seed, call counter, layer, site, global sequence index n, token t, column c) -- for
// the attention probabilities (head h, query t, key c) -- and of nothing else: no launch geometry, stream, precision mode or rank.
// The generator is Philox4x32-10 (Salmon et al., SC'11), written out here:
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (c >> 2, n, t | h << 16, (call counter & 0xffffff) << 8 | layer << 2 | site)
//   draw    = output word (c & 3) of the 10-round block
//   keep    = draw >= round(p * 2^32)  (p as float32), kept values scaled by 1 / (1 - p)
// One block yields the decisions of four adjacent columns; the kernels consume it whole.  include/cxrk.h restates the rule and
// tests/test_dropout_host.py restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>

namespace cxrk {

enum DropSite { DROP_EMBED = 0, DROP_ATTN_PROBS = 1, DROP_ATTN_OUT = 2, DROP_FFN_OUT = 3 };

struct DropKey {
  unsigned k0, k1;      // seed, low / high word
  unsigned c3;          // (call counter & 0xffffff) << 8 | layer << 2 | site
  unsigned thresh;      // keep iff draw >= thresh
  float scale;          // 1 / (1 - p)
  long row_offset;      // global sequence index of the first sequence of the tensor
  int rows_per_seq;     // rows of a hidden-site tensor per sequence: L, or 1 for the CLS rows of the last layer
};

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
    const unsigned lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c;
}

// keep factors (0 or 1/(1-p)) of columns 4*cg .. 4*cg+3 at sequence n, token / head word th = t | h << 16
__device__ __forceinline__ void drop_factors4(const DropKey& d, unsigned cg, unsigned n, unsigned th, float (&f)[4]) {
  const uint4 r = philox4x32_10(make_uint4(cg, n, th, d.c3), d.k0, d.k1);
  f[0] = r.x >= d.thresh ? d.scale : 0.f;
  f[1] = r.y >= d.thresh ? d.scale : 0.f;
  f[2] = r.z >= d.thresh ? d.scale : 0.f;
  f[3] = r.w >= d.thresh ? d.scale : 0.f;
}

// (n, t) of row `row` of a hidden-site tensor
__device__ __forceinline__ void drop_row(const DropKey& d, long row, unsigned& n, unsigned& t) {
  const long rps = d.rows_per_seq;
  n = (unsigned)(d.row_offset + row / rps);
  t = (unsigned)(row % rps);
}

}  // namespace cxrk
