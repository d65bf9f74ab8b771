// What the HOST decides about the matrix-product transforms of dft_mfma.h, and every fact the planner and the kernels must
// agree on, each written once: the plan of a map (transform size, tiling, operand sizes), the LDS layout (regions, pitches,
// sizes, the tail), what a wave and a thread can hold (accumulator tiles, window slots, spectrum items), the power-of-two scales
// and the choice of kernel instantiation.  Included by dft_mfma.h; needs DFT_HD of the hooks and nothing else, so a host program
// can include it on its own (tests/host/dft_plan_check.cpp).
#pragma once

#include <stddef.h>
#include <stdlib.h>

#ifndef DFT_HD
#define DFT_HD static inline      /* host + device helpers (the device build says __host__ __device__) */
#endif

namespace os2d_dft {

constexpr int DFT_THR = 512, DFT_WAVES = 8;
constexpr int DFT_G = 4;            // images per work-group iteration
constexpr int DFT_MAXP = 64;        // transform rows (P <= 64: the 2P rows of step 2 / step A are at most four 32-row tiles)
constexpr int DFT_MAXV = 48;        // half-spectrum columns (2V <= 96: three 32-column tiles; Q <= 94)
constexpr int DFT_MAXWK = 96;       // window columns rounded up to 16
constexpr int DFT_KREG = 8;         // k-steps of the register-resident operand (2 * Pp / 16 <= 8)
constexpr int DFT_LDS_MAX = 160 * 1024;      // LDS of a work-group (bytes)
// output forms of the inverse kernel (its ``zero_borders`` argument): split-fp16 activation units, the same + the zero border
// cells of the planes, or fp32 channel planes [pair][channel][H * W] scaled to <= 1 - what the forward kernel reads
constexpr int DFT_OUT_SHB = 0, DFT_OUT_SHB_BORDERS = 1, DFT_OUT_PLANES = 2;

// ---- capacity: what the kernels declare per wave and per thread (their arrays are sized by these; the planner admits a plan of
// 8 images only within them - dft_capacity_ok - and the plans of 4 images stay within them by the static_asserts below it)
constexpr int DFT_ACC_TILES = 3;                      // accumulator tiles (32 x 32) of a wave in one product
constexpr int DFT_SLOTS_G4 = 3, DFT_SLOTS_G8 = 2;     // window positions (row, 4 columns; all images) a thread prefetches
constexpr int DFT_ITEMS = 3;                          // spectrum items (image, v, 8 u) a thread prefetches

// ---- scales: exponents of the powers of two the operands carry (all exact; the "Scales" paragraph of dft_mfma.h)
constexpr int DFT_EX = 15;          // x * 2^15 (x <= 1)
constexpr int DFT_EF = 14;          // the DFT matrices FqT, Fp2, E2 * 2^14
constexpr int DFT_EGQ = 13;         // Gq * 2^13 (its entries reach 2)
constexpr int DFT_ER = 8;           // the row spectrum R * 2^8 (|R| <= window width <= 96)
constexpr int DFT_EY = 13;          // an image's largest |component| of Y is scaled into [2^DFT_EY, 2^(DFT_EY + 1))
constexpr double dft_pow2(int e) { return e >= 0 ? (double)(1 << e) : 1.0 / (double)(1 << -e); }
constexpr float DFT_SCALE_X = (float)dft_pow2(DFT_EX);                            // W phase
constexpr double DFT_SCALE_F = dft_pow2(DFT_EF), DFT_SCALE_GQ = dft_pow2(DFT_EGQ);      // dft_matrix_unit
constexpr float DFT_SCALE_R = (float)dft_pow2(DFT_ER - DFT_EX - DFT_EF);          // step 1's accumulators -> R * 2^8 (2^-21)
constexpr float DFT_SCALE_XOUT = (float)dft_pow2(-(DFT_ER + DFT_EF));             // step 2's accumulators -> X (2^-22)
constexpr float DFT_SCALE_PLANES = (float)dft_pow2(-DFT_EX);                      // DFT_OUT_PLANES: activations (<= 2^15) -> <= 1

struct DftPlan {
  int H, W;                        // map
  int P, Q, V, NBINS;              // transform size, V = Q/2 + 1; bins = v * P + u padded to a multiple of 8
  int T, TY, TX, TH, TW;           // overlap-save tiles (T = TY * TX = 1: the whole map in one transform)
  int oy, ox;                      // 3 along a tiled axis (window starts 3 cells before the tile; outputs sit at offset 3), else 0
  int LH, LW;                      // rows / columns of the window a tile loads (TH + 6 | H, TW + 6 | W)
  int RH;                          // rows of the inverse that are needed (oy + TH | H)
  int Pp;                          // P rounded up to 8: rows of a window in the operand arrays (k of step 2 / step A = 2 * Pp)
  int Wk;                          // LW rounded up to 16: k of step 1
  int N1;                          // 2 V rounded up to 32: columns of step 1
  int M2;                          // 2 P rounded up to 32: rows of step 2
  int Mx;                          // G * Pp rounded up to 32: rows of step 1 = (img, h)
  int N2;                          // G * V rounded up to 32: columns of step 2 / step A = (img, v)
  int MA;                          // 2 * RH rounded up to 32: rows of step A = (h, re | im)
  int MB;                          // G * (MA / 2) : rows of step B = (h, img)
  int KB;                          // 2 V rounded up to 16: k of step B
  int NBo;                         // columns of step B that are needed (ox + TW | W) rounded up to 32
  int G;                           // images per work-group iteration of both kernels: 4, or 8 for the small transforms (dft_plan_g8)
  int eT;                          // ceil(log2 P) + 1
  int fast;                        // 1: W % 4 == 0 and untiled (16-byte loads of the correlation rows)
  unsigned inv_cg, inv_t, inv_tx, inv_c4, inv_v, inv_pq, inv_og, inv_kg, inv_pp;   // ceil(2^32 / d) (0 where d == 1)
  // LDS (bytes)
  int lds_const, lds_union, lds_total;
};

DFT_HD constexpr int dft_round_up(int x, int m) { return (x + m - 1) / m * m; }
DFT_HD unsigned dft_magic(unsigned d) { return d > 1 ? (unsigned)(((1ull << 32) + d - 1) / d) : 0u; }

// sizes of the constant operand arrays of a (P, Q) transform, in 16-byte units: they depend on P and Q only, so every map
// (and every tiling) that uses the transform shares them
DFT_HD int dft_units_fqt(int P, int Q) { return (dft_round_up(Q, 16) / 8) * 2 * dft_round_up(Q + 2, 32); }
// P = 64 (radix 2 in the forward kernel): Fp2 is a block of DFT_R2_MATU units - the 64 x 32 real matrix of the 32-point transform
// [k group = 4][hi|lo][64 rows: cos | sin] in its first half, zeros behind it - followed by DFT_R2_TWU units of twiddles:
// float [32][re|im] = exp(-2 pi i u / 64)
constexpr int DFT_R2_P = 64, DFT_R2_MATU = 8 * 2 * 64, DFT_R2_TWU = 16;
DFT_HD bool dft_radix2(int P) { return P == DFT_R2_P; }
DFT_HD int dft_units_fp2(int P, int Q) {
  return dft_radix2(P) ? DFT_R2_MATU + DFT_R2_TWU : (2 * dft_round_up(P, 8) / 8) * 2 * dft_round_up(2 * P, 32);
}
DFT_HD int dft_units_e2(int P, int Q) { return (2 * dft_round_up(P, 8) / 8) * 2 * dft_round_up(2 * P, 32); }
DFT_HD int dft_units_gq(int P, int Q) { return (dft_round_up(Q + 2, 16) / 8) * 2 * dft_round_up(Q, 32); }
DFT_HD size_t dft_matrices_units(int P, int Q) {
  return (size_t)dft_units_fqt(P, Q) + dft_units_fp2(P, Q) + dft_units_e2(P, Q) + dft_units_gq(P, Q);
}

// ---- the LDS layout, for the planner (which budgets it) and the kernels (which address it):
//   [0, lds_const)           resident constants: FqT (forward) | Gq (inverse) and, with 8 images, the row operand Fp2 | E2 behind it
//   [lds_const, + lds_union) one after the other x | R2 | X staging (forward), Y2 | Tt (inverse)
//   [.., + DFT_TAIL_BYTES)   the tail: per-image maxima (inverse) | twiddles (forward, 64 rows)
// An operand array is [k / 8][hi | lo][pitch] units of 16 bytes; the arrays of the union region have one padding column.
DFT_HD int dft_lds_units(int k, int pitch) { return (k / 8) * 2 * pitch; }
DFT_HD int dft_lds_fqt(const DftPlan& pl) { return dft_lds_units(pl.Wk, pl.N1); }            // units: FqT [Wk / 8][2][N1]
DFT_HD int dft_lds_gq(const DftPlan& pl) { return dft_lds_units(pl.KB, pl.NBo); }            // units: Gq [KB / 8][2][NBo]
DFT_HD int dft_lds_rowop(int Pp, int rows) { return dft_lds_units(2 * Pp, rows); }           // units: Fp2 | E2 [2 Pp / 8][2][rows = M2]
DFT_HD int dft_pitch_x(const DftPlan& pl) { return pl.Mx + 1; }                              // units: x [Wk / 8][2][.]
DFT_HD int dft_pitch_n2(const DftPlan& pl) { return pl.N2 + 1; }                             // units: R2 | Y2 [2 Pp / 8][2][.]
DFT_HD int dft_pitch_tt(const DftPlan& pl) { return pl.MB + 1; }                             // units: Tt [KB / 8][2][.]
DFT_HD int dft_pitch_xs(int P, int G) { return P * 8 * G + 16; }      // BYTES per v of the X staging [v][u / 4][img][u % 4][re|im] (+ 16: banks)
DFT_HD int dft_lds_x_bytes(const DftPlan& pl) { return dft_lds_units(pl.Wk, dft_pitch_x(pl)) * 16; }
DFT_HD int dft_lds_n2_bytes(const DftPlan& pl) { return dft_lds_units(2 * pl.Pp, dft_pitch_n2(pl)) * 16; }      // R2 and Y2
DFT_HD int dft_lds_xs_bytes(const DftPlan& pl, int G) { return pl.V * dft_pitch_xs(pl.P, G); }
DFT_HD int dft_lds_tt_bytes(const DftPlan& pl) { return dft_lds_units(pl.KB, dft_pitch_tt(pl)) * 16; }
// the tail (bytes from its start): the inverse kernel's per-image maxima, float [DFT_WAVES][G], and the twiddles of the 64-row
// forward kernel, DFT_R2_TWU units
constexpr int DFT_TAIL_BYTES = 1024;
constexpr int DFT_TAIL_MAX = 0, DFT_TAIL_TW = 512;
constexpr int dft_tail_max_bytes(int G) { return DFT_WAVES * G * 4; }
static_assert(DFT_TAIL_MAX + dft_tail_max_bytes(8) <= DFT_TAIL_TW, "the maxima of 8 images end in front of the twiddles");
static_assert(DFT_TAIL_TW + DFT_R2_TWU * 16 <= DFT_TAIL_BYTES, "the twiddles end inside the tail");
// where the tail starts: as a byte offset (the planner's total) and as the kernels' pointer - the regions added to the LDS base
// one after the other: smem + (lds_const + lds_union) is different generated code in 15 kernels (profiles/dft_plan/isa_diff.md)
DFT_HD int dft_lds_tail(const DftPlan& pl) { return pl.lds_const + pl.lds_union; }
DFT_HD unsigned char* dft_lds_tail_ptr(unsigned char* smem, const DftPlan& pl) { return smem + pl.lds_const + pl.lds_union; }

// what the products and the prefetches of a plan count, against the capacity constants above
struct DftCounts {
  int t1, t2, tA, tB;              // tiles of step 1, 2, A, B
  int rows2, cols2;                // row tiles of step 2 / step A (the larger), column tiles of step 2 / step A
  int npos, nitem;                 // window positions, spectrum items per iteration
};
DFT_HD DftCounts dft_plan_counts(const DftPlan& pl) {
  DftCounts c;
  c.t1 = (pl.Mx / 32) * (pl.N1 / 32);
  c.t2 = (pl.M2 / 32) * (pl.N2 / 32);
  c.tA = (pl.MA / 32) * (pl.N2 / 32);
  c.tB = (pl.MB / 32) * (pl.NBo / 32);
  c.rows2 = (pl.M2 > pl.MA ? pl.M2 : pl.MA) / 32;
  c.cols2 = pl.N2 / 32;
  c.npos = pl.Pp * (pl.Wk / 4);
  c.nitem = pl.G * pl.V * (pl.Pp / 8);
  return c;
}
// 8 images: every product hands out tiles t = wave + DFT_WAVES j; 4 images: so do step 1 and step B, step 2 / step A keep row
// tile wave & 3 in registers and take column tiles (wave >> 2) + 2 j
DFT_HD bool dft_capacity_ok(const DftPlan& pl) {
  const DftCounts c = dft_plan_counts(pl);
  const int tiles = DFT_WAVES * DFT_ACC_TILES;
  if (c.t1 > tiles || c.tB > tiles || c.nitem > DFT_ITEMS * DFT_THR) return false;
  if (pl.G == 8) return c.t2 <= tiles && c.tA <= tiles && c.npos <= DFT_SLOTS_G8 * DFT_THR;
  return c.rows2 <= 4 && c.cols2 <= (DFT_WAVES / 4) * DFT_ACC_TILES && c.npos <= DFT_SLOTS_G4 * DFT_THR;
}
// 4 images: the limits of dft_plan_transform (P <= DFT_MAXP, V <= DFT_MAXV, Wk <= DFT_MAXWK; the output columns are a part of
// the window, NBo <= DFT_MAXWK) keep every plan within the capacity - no check at run time
static_assert(dft_round_up(DFT_G * DFT_MAXP, 32) / 32 <= DFT_WAVES && dft_round_up(2 * DFT_MAXV, 32) / 32 <= DFT_ACC_TILES,
              "step 1: at most 8 x 3 tiles");
static_assert(dft_round_up(2 * DFT_MAXP, 32) / 32 <= 4 && dft_round_up(DFT_G * DFT_MAXV, 32) / 32 <= (DFT_WAVES / 4) * DFT_ACC_TILES,
              "step 2 / step A: at most 4 row tiles, 6 column tiles reached as (wave >> 2) + 2 j");
static_assert(DFT_G * (dft_round_up(2 * DFT_MAXP, 32) / 2) / 32 <= DFT_WAVES && dft_round_up(DFT_MAXWK, 32) / 32 <= DFT_ACC_TILES,
              "step B: at most 8 x 3 tiles");
static_assert(dft_round_up(DFT_MAXP, 8) * (DFT_MAXWK / 4) <= DFT_SLOTS_G4 * DFT_THR, "window positions: at most 64 * 24");
static_assert(DFT_G * DFT_MAXV * (dft_round_up(DFT_MAXP, 8) / 8) <= DFT_ITEMS * DFT_THR, "spectrum items: at most 4 * 48 * 8");
static_assert(2 * dft_round_up(DFT_MAXP, 8) / 16 <= DFT_KREG, "k-steps of the register-resident operand");

// plan of ONE transform: window LH x LW -> P x Q, RH rows of the inverse needed, NBo output columns needed
static inline bool dft_plan_transform(int LH, int LW, int RH, int ncols, int minP, int minQ, int G, DftPlan* pl) {
  pl->G = G;
  pl->P = dft_round_up(minP, 4);
  // 60 rows pad to the operand arrays of 64 (Pp) anyway and would be the only other size with 8 k-steps in step 2 / step A: it
  // takes the 64-row transform, so that 8 k-steps always mean the radix-2 product (7 % more bins under the "exact" policy only)
  if (pl->P == 60) pl->P = DFT_R2_P;
  pl->Q = dft_round_up(minQ, 2);
  pl->V = pl->Q / 2 + 1;
  pl->NBINS = dft_round_up(pl->P * pl->V, 8);
  pl->LH = LH;
  pl->LW = LW;
  pl->RH = RH;
  pl->Pp = dft_round_up(pl->P, 8);
  pl->Wk = dft_round_up(LW, 16);
  pl->N1 = dft_round_up(2 * pl->V, 32);
  pl->M2 = dft_round_up(2 * pl->P, 32);
  pl->Mx = dft_round_up(G * pl->Pp, 32);
  pl->N2 = dft_round_up(G * pl->V, 32);
  pl->MA = dft_round_up(2 * RH, 32);
  pl->MB = G * (pl->MA / 2);
  pl->KB = dft_round_up(2 * pl->V, 16);
  pl->NBo = dft_round_up(ncols, 32);
  int e = 0;
  while ((1 << e) < pl->P) ++e;
  pl->eT = e + 1;
  if (pl->P > DFT_MAXP || pl->V > DFT_MAXV || pl->Wk > DFT_MAXWK || LH > pl->P || LW > pl->Q || RH > pl->P) return false;
  // LDS: constants FqT | Gq are resident (whichever kernel runs takes its own: the larger decides the common figure);
  // the union region holds, one after the other, x | R2 | X staging (forward) and Y2 | Tt (inverse)
  const int fqt = dft_lds_fqt(*pl) * 16, gq = dft_lds_gq(*pl) * 16;
  int u = dft_lds_x_bytes(*pl);
  if (dft_lds_n2_bytes(*pl) > u) u = dft_lds_n2_bytes(*pl);
  if (dft_lds_xs_bytes(*pl, G) > u) u = dft_lds_xs_bytes(*pl, G);
  if (dft_lds_tt_bytes(*pl) > u) u = dft_lds_tt_bytes(*pl);
  // EIGHT images per iteration (round 6): the fixed phases of an iteration - six barriers, the fill and drain of
  // four products, the burst of the next window's requests - do not shrink with the transform, so the small transforms of the
  // pyramid paid 1.3 - 1.9x per location.  With 8 images the products have 20 - 24 tiles (three per wave: the tile grids of
  // step 2 / step A no longer match the fixed "row tile in registers" ownership, so Fp2 / E2 live in LDS next to FqT / Gq
  // and every product takes the LDS-LDS path), the inverse kernel owns all 8 channels of an activation unit and writes whole
  // 16-byte units.  Fits the transforms up to 48 x 62.
  // (the 64-row transform keeps its half-size matrix in registers: 4 images)
  if (G == 8 && dft_radix2(pl->P)) return false;
  const int rowop = G == 8 ? dft_lds_rowop(pl->Pp, pl->M2) * 16 : 0;      // (E2 has M2 rows as well)
  pl->lds_const = (fqt > gq ? fqt : gq) + rowop;
  pl->lds_union = dft_round_up(u, 256);
  pl->lds_total = dft_lds_tail(*pl) + DFT_TAIL_BYTES;
  return pl->lds_total <= DFT_LDS_MAX && (G != 8 || dft_capacity_ok(*pl));
}

static inline void dft_set_tiles(DftPlan* pl, int H, int W, int TY, int TX, int TH, int TW) {
  pl->H = H;
  pl->W = W;
  pl->TY = TY;
  pl->TX = TX;
  pl->T = TY * TX;
  pl->TH = TH;
  pl->TW = TW;
  pl->oy = TY > 1 ? 3 : 0;
  pl->ox = TX > 1 ? 3 : 0;
  pl->fast = (pl->T == 1 && (W & 3) == 0) ? 1 : 0;
  pl->inv_t = dft_magic((unsigned)pl->T);
  pl->inv_tx = dft_magic((unsigned)TX);
  pl->inv_c4 = dft_magic((unsigned)(pl->Wk / 4));
  pl->inv_v = dft_magic((unsigned)pl->V);
  pl->inv_pq = dft_magic((unsigned)(pl->P / 4 * pl->G * 2));
  pl->inv_kg = dft_magic((unsigned)(pl->Pp / 8));
  pl->inv_pp = dft_magic((unsigned)pl->Pp);
}

// Transform sizes.  The weight spectra of the per-bin GEMM cost 0.24 MB per bin and transform size (654 MB for 64 x 84), and a
// dataset fed at its own aspect ratios and 7 pyramid scales meets hundreds of map sizes (reference os2d/data/dataloader.py:326,
// os2d/config.py:194).  Since every map can be cut into overlap-save tiles, the planner may restrict itself to a handful of
// CANONICAL sizes and pay in bins instead of in resident spectra (35.6 GB cached for 52 FFT-friendly sizes):
//   policy 1 (default)  the six sizes below - the exact transforms of the 7-scale pyramid of a 1280 x 960 image (levels 30x40 ..
//                       60x80 whole, 72x96 / 84x112 / 96x128 as 2 x 2 tiles): 10,220 bins = 2.4 GB of weight spectra in total
//   policy 0            any P % 4 == 0, even Q: the smallest transform per map (fewest bins; one set of spectra per size)
// $OS2D_DFT_SIZES = canonical | exact selects it for the process (read once).
struct DftSize {
  int P, Q;
};
static const DftSize DFT_CANONICAL[6] = {{36, 46}, {44, 54}, {48, 62}, {52, 68}, {56, 70}, {64, 84}};

// The whole map in one transform when it fits (P >= H + 3, Q >= W + 3: the zero padding is the halo), otherwise the tiling
// with the fewest bins in total; an axis is either untiled or cut into >= 2 tiles of ceil(n / k) outputs whose window is 6
// longer.
static inline bool dft_make_plan_policy(int H, int W, int canonical, DftPlan* out, int G = DFT_G) {
  bool found = false;
  long best = 0;
  for (int TY = 1; TY <= 48; ++TY)
    for (int TX = 1; TX <= 48; ++TX) {
      const int TH = (H + TY - 1) / TY, TW = (W + TX - 1) / TX;
      if ((TY > 1 && (TY - 1) * TH >= H) || (TX > 1 && (TX - 1) * TW >= W)) continue;     // an empty last tile
      const int LH = TY > 1 ? TH + 6 : H, LW = TX > 1 ? TW + 6 : W;
      const int minP = TY > 1 ? TH + 6 : H + 3, minQ = TX > 1 ? TW + 6 : W + 3;
      if (minP > DFT_MAXP || minQ > 2 * (DFT_MAXV - 1)) continue;
      for (int k = 0; k < (canonical ? 6 : 1); ++k) {
        if (canonical && (DFT_CANONICAL[k].P < minP || DFT_CANONICAL[k].Q < minQ)) continue;
        DftPlan c = {};
        if (!dft_plan_transform(LH, LW, TY > 1 ? TH + 3 : H, TX > 1 ? TW + 3 : W, canonical ? DFT_CANONICAL[k].P : minP,
                                canonical ? DFT_CANONICAL[k].Q : minQ, G, &c))
          continue;
        dft_set_tiles(&c, H, W, TY, TX, TH, TW);
        const long cost = (long)c.T * c.NBINS;
        if (!found || cost < best) {
          found = true;
          best = cost;
          *out = c;
        }
      }
    }
  return found;
}

#ifndef OS2D_HOST_EMU
static inline int dft_size_policy() {
  static const int policy = [] {
    const char* e = getenv("OS2D_DFT_SIZES");
    return (e && (e[0] == 'e' || e[0] == '0')) ? 0 : 1;
  }();
  return policy;
}
#else
static inline int dft_size_policy() { return emu_dft_policy; }
#endif
static inline bool dft_make_plan(int H, int W, DftPlan* out) { return dft_make_plan_policy(H, W, dft_size_policy(), out); }
// The plan of the same map with 8 images per iteration: the SAME tiling and transform size as ``base`` (= dft_make_plan: the spectra
// layouts do not depend on G), its own operand sizes; false when the transform is too large for it (then both kernels take 4).
static inline bool dft_plan_g8(const DftPlan& base, DftPlan* out) {
  DftPlan c = {};
  if (!dft_plan_transform(base.LH, base.LW, base.RH, base.TX > 1 ? base.TW + 3 : base.W, base.P, base.Q, 8, &c)) return false;
  dft_set_tiles(&c, base.H, base.W, base.TY, base.TX, base.TH, base.TW);
  *out = c;
  return true;
}

// Which instantiation of the kernels a plan takes: the k-steps of the product whose row operand lives in registers (step 2 /
// step A: 2 Pp / 16) as a template parameter where that is 5 .. 8 - the canonical transform sizes - else 0 = any count behind
// uniform guards; 8 images (row operand in LDS): always 0.  DFT_R2_KS k-steps are the 64-row transform and nothing else
// (dft_plan_transform): the forward kernel of that instantiation is the radix-2 form.
constexpr int DFT_R2_KS = 2 * DFT_R2_P / 16;
static_assert(DFT_R2_KS == DFT_KREG, "the 64-row transform is the largest one");
DFT_HD int dft_ksteps_param(const DftPlan& pl) {
  const int ks = 2 * pl.Pp / 16;
  return pl.G != 8 && ks >= 5 && ks <= DFT_KREG ? ks : 0;
}

// Spectra in quads of bins, BLOCKED by 64 pairs (the pair tile of the per-bin GEMM):
//   [pair' / 64][bins / 4][pair' % 64][channel stride][4] complex64, the last block holding NBT % 64 pairs (no padding: the
//   buffers keep their size NBT x bins x channels).
// With one block - up to 64 pairs - this is [bins / 4][pair'][channel][4].  With 1024 pairs the quads of one pair were 7.6 MB
// (X) / 4 MB (Y) apart: every 128-byte run of a transform iteration in its own DRAM page and translation entry; blocked, the
// distance is that of the 64-pair case (475 / 262 KB) whatever the batch, and a GEMM work-group's operands are one contiguous
// slab.  Returns the float offset of (pair', quad 0, channel 0); *qstride = floats between consecutive quads of that pair.
constexpr int DFT_PBLK = 64;
DFT_HD size_t dft_spectra_pair0(int pr, int NBT, int NQ, int cstride, size_t* qstride) {
  const int pb = pr / DFT_PBLK, pl = pr - pb * DFT_PBLK;
  const int nbl = NBT - pb * DFT_PBLK < DFT_PBLK ? NBT - pb * DFT_PBLK : DFT_PBLK;
  *qstride = (size_t)nbl * cstride * 8;
  return ((size_t)pb * DFT_PBLK * NQ + pl) * cstride * 8;
}

}  // namespace os2d_dft
