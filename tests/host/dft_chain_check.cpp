// Host check of the register hand-over in the 64-row forward kernel of os2d_amd/csrc/dft_mfma.h - step 1's accumulators become the
// B operand of step 2 without passing through LDS, the complex combination is a lane swap - on the SPMD emulator (spmd_emu.h)
// against a float64 DFT.
// The 61 x 81 map (the largest untiled window, a width that takes the 4-byte aligned loads) on its 64 x 84 transform, one pair:
//   1. the row operand of step 2 as dft_matrix_unit builds it: 32 rows of cosines and 32 of sines of the 32-point transform, the
//      k order inside k-step a, half-wave hw, element t being h' = 8 (2 a + t / 4) + 4 hw + t % 4 - stated here on its own -
//      hi + lo within 2^-21 of the float64 value (two fp16 roundings of a number below 2^14), the rest of the block zero
//   2. C = 5 channels: one work-group runs two iterations, the second with ONE live channel (a ragged group) - every bin of
//      every channel against float64, the padding bins and the channels beyond C exactly zero
//   3. C = 4 channels (one iteration): its spectra equal the first four channels of 2. bit for bit
// Bound: that of dft_radix2_check.cpp for the same arithmetic, 2e-6 max|X| + 1e-5.
// Built and run by tests/test_dft_chain_host.py.
#include <cstring>

#define DFT_EMU_POLICY 1      // the canonical sizes
#include "dft_emu.h"      // the hooks on the emulator, dft_mfma.h, spec_index, table, frand

using namespace os2d_dft;

constexpr int H = 61, W = 81, NB = 1, CPAD = 8, HW = H * W;

static double half_at(const u32x4& unit, int t) {
  const unsigned w = unit[t >> 1];
  const unsigned short b = (unsigned short)((t & 1) ? (w >> 16) : (w & 0xffffu));
  return (double)__builtin_bit_cast(_Float16, b);
}

int main() {
  DftPlan pl;
  if (!dft_make_plan(H, W, &pl) || pl.P != 64 || pl.Q != 84 || pl.T != 1 || pl.fast != 0 || !dft_radix2(pl.P)) {
    std::printf("the 61x81 map is not on the untiled 64 x 84 plan with unaligned rows\nFAILED\n");
    return 1;
  }
  const int P = pl.P, Q = pl.Q, V = pl.V, NQ = pl.NBINS / 4;
  const std::vector<double> tp = table(P), tq = table(Q);
  const int nf = dft_units_fqt(P, Q), n2 = dft_units_fp2(P, Q);
  std::vector<u32x4> mats((size_t)nf + n2);
  for (int i = 0; i < nf; ++i) dft_matrix_unit(0, i, P, Q, tp.data(), tq.data(), &mats[i]);
  for (int i = 0; i < n2; ++i) dft_matrix_unit(1, i, P, Q, tp.data(), tq.data(), &mats[nf + i]);
  const u32x4 *FqT = mats.data(), *Fp2 = FqT + nf;
  int rc = 0;

  // ---------------- 1. the permuted row operand
  {
    double worst = 0.0;
    int nonzero_tail = 0;
    for (int a = 0; a < 2; ++a)
      for (int hw = 0; hw < 2; ++hw)
        for (int row = 0; row < 64; ++row)
          for (int t = 0; t < 8; ++t) {
            const int h = 8 * (2 * a + t / 4) + 4 * hw + t % 4, u = row & 31;
            const double ang = 2.0 * M_PI * ((u * h) % 32) / 32.0;
            const double want = (row < 32 ? std::cos(ang) : std::sin(ang)) * 16384.0;
            const double got = half_at(Fp2[((2 * a + hw) * 2 + 0) * 64 + row], t) + half_at(Fp2[((2 * a + hw) * 2 + 1) * 64 + row], t);
            worst = std::fmax(worst, std::fabs(got - want) / 16384.0);
          }
    for (int i = 4 * 2 * 64; i < DFT_R2_MATU; ++i)
      for (int t = 0; t < 4; ++t) nonzero_tail += Fp2[i][t] != 0u;
    std::printf("operand: 64 x 32, max |hi + lo - float64| = %.3e of the scale (bound %.3e), %d non-zero words behind it\n", worst,
                std::ldexp(1.0, -21), nonzero_tail);
    if (!(worst <= std::ldexp(1.0, -21)) || nonzero_tail) std::printf("OPERAND MISMATCH\n"), rc = 1;
  }

  // ---------------- 2. / 3. forward with 5 and with 4 channels of the same input
  unsigned seed = 977u;
  constexpr int CMAX = 5;
  std::vector<float> corr5((size_t)CMAX * HW), invn((size_t)HW);
  for (auto& v : corr5) v = (float)(frand(seed) * 2.0 - 0.7);
  for (auto& v : invn) v = (float)(0.2 + 0.5 * frand(seed));          // relu(corr) * invn <= 1.3 * 0.7 < 1
  auto run = [&](int C, std::vector<float>& X) {
    X.assign((size_t)NQ * NB * CPAD * 8, 777.0f);
    DftPlan fp = pl;
    const int CG = (C + 3) / 4, iters = NB * CG;
    fp.inv_cg = dft_magic((unsigned)CG);
    emu::launch(1, 512, fp.lds_total,
                [&] { dft_forward_body<false, false, 4, 8, 8>(corr5.data(), invn.data(), X.data(), FqT, Fp2, fp, C, CPAD, NB, iters); });
  };
  std::vector<float> X5, X4;
  run(5, X5);
  run(4, X4);

  double worst = 0.0, scale = 0.0;
  for (int c = 0; c < CMAX; ++c) {
    std::vector<double> xi((size_t)HW);
    for (int i = 0; i < HW; ++i) xi[i] = (double)(std::fmax(corr5[(size_t)c * HW + i], 0.f) * invn[i]);
    std::vector<double> rr((size_t)H * V), ri((size_t)H * V);
    for (int r = 0; r < H; ++r)
      for (int v = 0; v < V; ++v) {
        double sr = 0, si = 0;
        for (int w = 0; w < W; ++w) {
          const int a = (v * w) % Q;
          sr += xi[r * W + w] * tq[2 * a];
          si += xi[r * W + w] * tq[2 * a + 1];
        }
        rr[(size_t)r * V + v] = sr;
        ri[(size_t)r * V + v] = si;
      }
    for (int u = 0; u < P; ++u)
      for (int v = 0; v < V; ++v) {
        double sr = 0, si = 0;
        for (int r = 0; r < H; ++r) {
          const int a = (u * r) % P;
          const double cr = tp[2 * a], ci = tp[2 * a + 1];
          sr += rr[(size_t)r * V + v] * cr - ri[(size_t)r * V + v] * ci;
          si += rr[(size_t)r * V + v] * ci + ri[(size_t)r * V + v] * cr;
        }
        const float* got = &X5[spec_index(v * P + u, 0, NB, NQ, CPAD, c)];
        worst = std::fmax(worst, std::fmax(std::fabs(got[0] - sr), std::fabs(got[1] - si)));
        scale = std::fmax(scale, std::fmax(std::fabs(sr), std::fabs(si)));
      }
    for (int bin = P * V; bin < pl.NBINS; ++bin) {
      const float* got = &X5[spec_index(bin, 0, NB, NQ, CPAD, c)];
      if (got[0] != 0.f || got[1] != 0.f) std::printf("padding bin %d not zero\n", bin), rc = 1;
    }
  }
  for (int c = CMAX; c < CPAD; ++c)      // channels 5 .. 7 belong to the second (ragged) channel group: zeros
    for (int bin = 0; bin < pl.NBINS; ++bin) {
      const float* got = &X5[spec_index(bin, 0, NB, NQ, CPAD, c)];
      if (got[0] != 0.f || got[1] != 0.f) {
        std::printf("channel %d beyond C: bin %d not zero\n", c, bin);
        rc = 1;
        break;
      }
    }
  const double bound = 2e-6 * scale + 1e-5;
  std::printf("forward: max |X - float64| = %.3e (largest |X| %.1f, bound %.3e)\n", worst, scale, bound);
  if (!(worst <= bound)) std::printf("FORWARD MISMATCH\n"), rc = 1;

  size_t differ = 0;
  for (int c = 0; c < 4; ++c)
    for (int bin = 0; bin < pl.NBINS; ++bin)
      differ += std::memcmp(&X4[spec_index(bin, 0, NB, NQ, CPAD, c)], &X5[spec_index(bin, 0, NB, NQ, CPAD, c)], 8) != 0;
  std::printf("4 channels against the first four of 5: %zu bins differ\n", differ);
  if (differ) std::printf("CHANNEL GROUP MISMATCH\n"), rc = 1;

  std::printf(rc ? "FAILED\n" : "ok\n");
  return rc;
}
