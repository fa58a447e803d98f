// 2:4-sparse near tiles for the one-wave matrix-pipe FISTA form (fista_mfma.h), for v_smfmac_f32_16x16x64_f16: one
// instruction whose A operand is 16 x 64 at 2:4 sparsity (two kept values in every aligned group of four k) carries BOTH
// near tiles of a block, 6 matrix instructions per block and pass instead of 12.  Host and device build the tiles from
// the same functions; the host side is what tests/test_sparse_tiles_host.py checks (through pb_mfma_sparse_tile).
//
// The form.  With 31-sample blocks, the sum slot and K <= 33 taps the dense kernel computes
//   x_q = C0 w_q + C1 w_{q-1} + S sum_{b <= q-2} w_b,
// and most of C1 equals S = c[K-1]: the row [C0 | C1] is dense.  The running prefix D_q = 2^-9 sum_{b <= q-1} w_b sits in
// block q's OWN sum slot before its products run, so the far field can start one block closer:
//   x_q = C0 w_q - E w_{q-1} + S sum_{b <= q-1} w_b,      E[ko][ki] = S - c[31 + ko - ki],
// with input column 31 of C0 (the block's own sum slot) carrying S 2^9.  E is zero unless ki >= ko + 33 - K, and its
// column 31 is zero (the previous block's sum slot is no input).  C0 is zero for ki > ko apart from the sum row and the
// sum column.  For K <= 32 the four entries {C0[ko][2p], C0[ko][2p+1], E[ko][2p], E[ko][2p+1]} of any row ko and pair p
// hold at most two nonzeros: ko = 2p: c[0] and E[ko][ko+1]; ko = 2p+1: two of C0, none of E; ko > 2p+1: two of C0;
// ko < 2p: two of E; the sum row: 2^-9 twice (pair 15: 2^-9 and 1); pair 15 of a real row: S 2^9 and one of c[0] (ko = 30)
// or E[ko][30].  At K = 33 the diagonal of E is nonzero, three in a group: K = 33 stays on the dense tiles.
// The adjoint mirrors it: g_q = C0^T r_q - E^T r_{q+1} + S sum_{b >= q+1} r_b, the suffix sum in block q's own slot.
//
// Column order.  The B operand of the instruction is 64 x 16, 8 registers of two halves per lane (n = lane & 15,
// g = lane >> 4); registers 2t, 2t+1 of a lane are one aligned group of four k.  Register 2t + e holds pair t (slots
// 8g + 2t, 8g + 2t + 1) of the block of PARITY e: every group of four is one pair of block q and the same pair of its
// neighbour, block q+1 overwrites the registers of block q-1 only, and a fragment is written once and serves as "own"
// and then as "other".  Hence two tiles per pass and row half: which parity is "own" alternates with q.
//   position 2 e + s of the group (g, t)   <->   slot 8 g + 2 t + s of the block of parity e
// The A operand holds, per lane (row rho = lane & 15, kg = lane >> 4), 8 kept values and one 16-bit word of 2-bit
// positions; values 2p, 2p+1 and bits [4p+1:4p], [4p+3:4p+2] belong to the group that B holds in lane group
// g = 2 (kg & 1) + (p >> 1) as t = 2 (kg >> 1) + (p & 1) (measured: tools/microbench/smfmac_layout.hip).
#pragma once
#include "mfma_core.h"

namespace pb {

constexpr int SPARSE_TILE_KMAX = 32;

// one entry of the joined tile [own | other] of a pass (0: forward, 1: adjoint): output slot ko, input slot ki of the
// block itself (own) or of its neighbour (forward: the block before; adjoint: the block behind).  cval(lag) = c[lag] for
// 0 <= lag <= 63 (c[63] = S) and 0 for lag < 0.
template <typename CV>
__host__ __device__ __forceinline__ float sparse_tile_entry(CV&& cval, int pass, bool own, int ko, int ki) {
  const float S = cval(63);
  const int d = pass == 0 ? ko - ki : ki - ko;
  if (own) {
    if (ko == 31) return ki == 31 ? 1.0f : 1.0f / (float)(1 << 9);
    if (ki == 31) return S * (float)(1 << 9);
    return cval(d);
  }
  if (ko == 31 || ki == 31) return 0.0f;
  return cval(31 + d) - S;                       // -E
}

// what lane `lane` holds of the tile (pass, par: the parity of the block whose products use it, r: row half): its 8
// compressed values and its 16 position bits.  False if a group holds more than two nonzeros (K > 32).
template <typename CV>
__host__ __device__ __forceinline__ bool sparse_tile_lane(CV&& cval, int pass, int par, int r, int lane, float (&val)[8], unsigned& idx) {
  const int rho = lane & 15, kg = lane >> 4, ko = 8 * (rho >> 2) + 4 * r + (rho & 3);
  bool ok = true;
  idx = 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int gb = 2 * (kg & 1) + (p >> 1), t = 2 * (kg >> 1) + (p & 1);      // the group of four as the B operand holds it
    float d[4];
#pragma unroll
    for (int pos = 0; pos < 4; ++pos) d[pos] = sparse_tile_entry(cval, pass, (pos >> 1) == par, ko, 8 * gb + 2 * t + (pos & 1));
    const bool n0 = d[0] != 0.0f, n1 = d[1] != 0.0f, n2 = d[2] != 0.0f, n3 = d[3] != 0.0f;
    ok = ok && ((int)n0 + (int)n1 + (int)n2 + (int)n3 <= 2);
    int i0 = n0 ? 0 : (n1 ? 1 : (n2 ? 2 : 3));   // the first nonzero and the last one ...
    int i1 = n3 ? 3 : (n2 ? 2 : (n1 ? 1 : 0));
    if (i0 >= i1) {                              // ... one or none: a zero beside it (positions ascending and distinct)
      const bool none = !(n0 || n1 || n2 || n3);
      const int z = i0;
      i0 = none ? 0 : (z < 3 ? z : 2);
      i1 = none ? 1 : (z < 3 ? z + 1 : 3);
    }
    val[2 * p] = i0 == 0 ? d[0] : (i0 == 1 ? d[1] : d[2]);
    val[2 * p + 1] = i1 == 1 ? d[1] : (i1 == 2 ? d[2] : d[3]);
    idx |= (unsigned)(i0 | (i1 << 2)) << (4 * p);
  }
  return ok;
}

// ---- host side: the whole tile, split in float16 hi = RTZ(x) and lo = RNE(x - hi) as the kernels split (mfma_core.h) ----
inline unsigned short host_f16_bits(_Float16 h) { return __builtin_bit_cast(unsigned short, h); }
inline _Float16 host_f16_rtz(float x) {
  _Float16 h = (_Float16)x;                      // round to nearest even ...
  if (fabsf((float)h) > fabsf(x)) {              // ... one step back towards zero where that went outwards
    h = __builtin_bit_cast(_Float16, (unsigned short)(host_f16_bits(h) - 1));
  }
  return h;
}

// hi, lo: [16][32] float16 bits, row rho, kept value 8 kg + j of lane group kg; idx: [16][4] position words, row rho, lane group kg.
// Returns 0, or 1 if K is outside 1 .. 32 (or a group of the tile holds more than two nonzeros).
inline int build_sparse_tile_host(const MfmaTaps& tp, int K, int pass, int par, int r, unsigned short* hi, unsigned short* lo, unsigned short* idx) {
  if (K < 1 || K > SPARSE_TILE_KMAX) return 1;
  auto cval = [&](int lag) -> float { return lag < 0 ? 0.0f : tp.c[lag > 63 ? 63 : lag]; };
  for (int lane = 0; lane < 64; ++lane) {
    float val[8];
    unsigned ix;
    if (!sparse_tile_lane(cval, pass, par, r, lane, val, ix)) return 1;
    const int rho = lane & 15, kg = lane >> 4;
    for (int j = 0; j < 8; ++j) {
      const _Float16 h = host_f16_rtz(val[j]);
      const _Float16 l = (_Float16)(val[j] - (float)h);
      hi[rho * 32 + 8 * kg + j] = host_f16_bits(h);
      lo[rho * 32 + 8 * kg + j] = host_f16_bits(l);
    }
    idx[rho * 4 + kg] = (unsigned short)ix;
  }
  return 0;
}

}  // namespace pb
