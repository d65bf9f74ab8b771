// Host check of the 64-row plan of os2d_amd/csrc/dft_mfma.h - the forward kernel with the radix-2 column transform (two 32-point
// products and a butterfly in step 2) and the inverse kernel that reads its spectra - on the SPMD emulator (spmd_emu.h) against
// float64 DFTs.
// The 60 x 80 map on its 64 x 84 transform, 2 pairs, 5 channels forward (a partial channel group), 8 output channels inverse:
//   1. the forward spectra against a float64 DFT of the same window
//   2. the inverse output for GIVEN spectra (a wide dynamic range, as tests/host/dft_mfma_check.cpp feeds it) against float64
//   3. the round trip: the spectra of 1. through the inverse kernel give the window back
//   4. the scale bound: one image whose spectrum has Y[u] = -Y[u + 32], re = +-im, every component of the largest magnitude the
//      per-image scale can meet (mantissa of ones: m s = 2^14 (1 - 2^-24)) - a butterfly in front of step A would form components
//      of 2 sqrt(2) m from it, the largest it can; whatever form step A takes, they must stay inside fp16 (range flag clear) and
//      the output must still match float64.
// Bounds: those of dft_mfma_check.cpp for the same arithmetic (fp16 hi + lo operands, fp32 accumulation): forward
// 2e-6 max|X| + 1e-5, inverse 1.5e-6 of the channel's largest output; the round trip is bounded by their sum (every bin off by the
// forward bound moves an output by at most that bound: the inverse averages P Q bins).
// Built and run by tests/test_dft_radix2_host.py.
#define DFT_EMU_POLICY 1      // the canonical sizes
#include "dft_emu.h"      // the hooks on the emulator, dft_mfma.h, spec_index, table, frand, ws_of / base_of / plane_of

using namespace os2d_dft;

constexpr int H = 60, W = 80, NB = 2, C = 5, CPAD = 8, COUT = 8, MTP = 128, HW = H * W, GRID = 2;

struct Setup {
  DftPlan pl;
  std::vector<double> tp, tq;
  std::vector<u32x4> mats;
  const u32x4 *FqT, *Fp2, *E2, *Gq;
};

// float64 inverse of the spectra of (pair, channel o) -> y[h][w], the untiled 60 x 80 window
static void inverse64(const Setup& s, const std::vector<float>& Y, int pair, int o, std::vector<double>& y) {
  const int P = s.pl.P, Q = s.pl.Q, V = s.pl.V;
  y.assign((size_t)HW, 0.0);
  std::vector<double> tr(V), ti(V);
  for (int h = 0; h < H; ++h) {
    for (int v = 0; v < V; ++v) {
      double sr = 0, si = 0;
      for (int u = 0; u < P; ++u) {
        const float* c = &Y[spec_index(v * P + u, pair, NB, s.pl.NBINS / 4, COUT, o)];
        const int a = (u * h) % P;
        const double cr = s.tp[2 * a], ci = -s.tp[2 * a + 1];
        sr += c[0] * cr - c[1] * ci;
        si += c[0] * ci + c[1] * cr;
      }
      tr[v] = sr;
      ti[v] = si;
    }
    for (int w = 0; w < W; ++w) {
      double s2 = 0;
      for (int v = 0; v < V; ++v) {
        const double a_v = (v == 0 || 2 * v == Q) ? 1.0 : 2.0;
        const int a = (v * w) % Q;
        s2 += a_v * (tr[v] * s.tq[2 * a] + ti[v] * s.tq[2 * a + 1]);
      }
      y[(size_t)h * W + w] = s2 / ((double)P * Q);
    }
  }
}

// the inverse kernel on spectra Y with bias / output scale bp -> values [NB][COUT][H][W] (hi + lo, divided by the scale again)
static int run_inverse(const Setup& s, const std::vector<float>& Y, const std::vector<float>& bp, std::vector<double>& got) {
  const int PLANE = plane_of(H, W), Ws = ws_of(W), BASE = base_of(W);
  std::vector<unsigned char> out((size_t)NB * (COUT / 8) * 2 * PLANE * 16, 0x5A);
  int flag = 0;
  DftPlan ip = s.pl;
  const int OG = COUT / 4, iters = NB * OG;
  ip.inv_og = dft_magic((unsigned)OG);
  emu::launch(GRID, DFT_THR, ip.lds_total,
              [&] { dft_inverse_body<false, 8>(Y.data(), bp.data(), MTP, out.data(), s.E2, s.Gq, ip, COUT, NB, PLANE, Ws, BASE, iters, &flag, 1); });
  got.assign((size_t)NB * COUT * HW, 0.0);
  for (int nb = 0; nb < NB; ++nb)
    for (int o = 0; o < COUT; ++o) {
      const unsigned char* hi = &out[(((size_t)nb * (COUT / 8) + (o >> 3)) * 2 + 0) * (size_t)PLANE * 16];
      const unsigned char* lo = &out[(((size_t)nb * (COUT / 8) + (o >> 3)) * 2 + 1) * (size_t)PLANE * 16];
      for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w) {
          const size_t cell = (size_t)BASE + (size_t)h * Ws + w;
          const _Float16 hv = *reinterpret_cast<const _Float16*>(hi + cell * 16 + (o & 7) * 2);
          const _Float16 lv = *reinterpret_cast<const _Float16*>(lo + cell * 16 + (o & 7) * 2);
          got[((size_t)nb * COUT + o) * HW + (size_t)h * W + w] = ((double)hv + (double)lv) / (double)bp[2 * MTP + o];
        }
    }
  return flag;
}

int main() {
  Setup s;
  if (!dft_make_plan(H, W, &s.pl) || s.pl.P != 64 || s.pl.Q != 84 || s.pl.T != 1 || 2 * s.pl.Pp / 16 != 8 || !dft_radix2(s.pl.P)) {
    std::printf("the 60x80 map is not on the 64 x 84 radix-2 plan\nFAILED\n");
    return 1;
  }
  const int P = s.pl.P, Q = s.pl.Q, V = s.pl.V, NQ = s.pl.NBINS / 4;
  s.tp = table(P);
  s.tq = table(Q);
  s.mats.resize(dft_matrices_units(P, Q));
  const int nf = dft_units_fqt(P, Q), n2 = dft_units_fp2(P, Q), ne = dft_units_e2(P, Q), ng = dft_units_gq(P, Q);
  for (int i = 0; i < nf; ++i) dft_matrix_unit(0, i, P, Q, s.tp.data(), s.tq.data(), &s.mats[i]);
  for (int i = 0; i < n2; ++i) dft_matrix_unit(1, i, P, Q, s.tp.data(), s.tq.data(), &s.mats[nf + i]);
  for (int i = 0; i < ne; ++i) dft_matrix_unit(2, i, P, Q, s.tp.data(), s.tq.data(), &s.mats[nf + n2 + i]);
  for (int i = 0; i < ng; ++i) dft_matrix_unit(3, i, P, Q, s.tp.data(), s.tq.data(), &s.mats[nf + n2 + ne + i]);
  s.FqT = s.mats.data(), s.Fp2 = s.FqT + nf, s.E2 = s.Fp2 + n2, s.Gq = s.E2 + ne;
  std::printf("plan P=%d Q=%d bins=%d, half-size forward matrix of %d units (+ %d of twiddles)\n", P, Q, s.pl.NBINS, DFT_R2_MATU, DFT_R2_TWU);
  int rc = 0;

  // ---------------- 1. forward
  unsigned seed = 4242u;
  std::vector<float> corr((size_t)NB * C * HW), invn((size_t)NB * HW);
  for (auto& v : corr) v = (float)(frand(seed) * 2.0 - 0.7);
  for (auto& v : invn) v = (float)(0.2 + 0.5 * frand(seed));          // relu(corr) * invn <= 1.3 * 0.7 < 1
  std::vector<float> X((size_t)NQ * NB * CPAD * 8, 777.0f);
  {
    DftPlan fp = s.pl;
    const int CG = (C + 3) / 4, iters = NB * CG;
    fp.inv_cg = dft_magic((unsigned)CG);
    emu::launch(GRID, 512, fp.lds_total,
                [&] { dft_forward_body<false, true, 4, 8, 8>(corr.data(), invn.data(), X.data(), s.FqT, s.Fp2, fp, C, CPAD, NB, iters); });
  }
  std::vector<double> x((size_t)NB * C * HW);
  double fwd_worst = 0.0, fwd_scale = 0.0, xmax = 0.0;
  for (int nb = 0; nb < NB; ++nb)
    for (int c = 0; c < C; ++c) {
      double* xi = &x[((size_t)nb * C + c) * HW];
      for (int i = 0; i < HW; ++i) {
        xi[i] = (double)(std::fmax(corr[((size_t)nb * C + c) * HW + i], 0.f) * invn[(size_t)nb * HW + i]);
        xmax = std::fmax(xmax, xi[i]);
      }
      std::vector<double> rr((size_t)H * V), ri((size_t)H * V);
      for (int r = 0; r < H; ++r)
        for (int v = 0; v < V; ++v) {
          double sr = 0, si = 0;
          for (int w = 0; w < W; ++w) {
            const int a = (v * w) % Q;
            sr += xi[r * W + w] * s.tq[2 * a];
            si += xi[r * W + w] * s.tq[2 * a + 1];
          }
          rr[(size_t)r * V + v] = sr;
          ri[(size_t)r * V + v] = si;
        }
      for (int u = 0; u < P; ++u)
        for (int v = 0; v < V; ++v) {
          double sr = 0, si = 0;
          for (int r = 0; r < H; ++r) {
            const int a = (u * r) % P;
            const double cr = s.tp[2 * a], ci = s.tp[2 * a + 1];
            sr += rr[(size_t)r * V + v] * cr - ri[(size_t)r * V + v] * ci;
            si += rr[(size_t)r * V + v] * ci + ri[(size_t)r * V + v] * cr;
          }
          const float* got = &X[spec_index(v * P + u, nb, NB, NQ, CPAD, c)];
          fwd_worst = std::fmax(fwd_worst, std::fmax(std::fabs(got[0] - sr), std::fabs(got[1] - si)));
          fwd_scale = std::fmax(fwd_scale, std::fmax(std::fabs(sr), std::fabs(si)));
        }
      for (int bin = P * V; bin < s.pl.NBINS; ++bin) {
        const float* got = &X[spec_index(bin, nb, NB, NQ, CPAD, c)];
        if (got[0] != 0.f || got[1] != 0.f) std::printf("padding bin %d not zero\n", bin), rc = 1;
      }
    }
  for (int nb = 0; nb < NB; ++nb)      // channels 5 .. 7 belong to the second (partial) channel group: zeros
    for (int c = C; c < CPAD; ++c)
      for (int bin = 0; bin < s.pl.NBINS; ++bin) {
        const float* got = &X[spec_index(bin, nb, NB, NQ, CPAD, c)];
        if (got[0] != 0.f || got[1] != 0.f) {
          std::printf("channel %d beyond C: bin %d not zero\n", c, bin);
          rc = 1;
          bin = s.pl.NBINS;
        }
      }
  const double fwd_bound = 2e-6 * fwd_scale + 1e-5;
  std::printf("forward: max |X - float64| = %.3e (largest |X| %.1f, bound %.3e)\n", fwd_worst, fwd_scale, fwd_bound);
  if (!(fwd_worst <= fwd_bound)) std::printf("FORWARD MISMATCH\n"), rc = 1;

  // ---------------- 2. inverse of given spectra + 4. the scale bound (pair 0, channel 0)
  {
    std::vector<float> Y((size_t)NQ * NB * COUT * 8);
    for (size_t i = 0; i < Y.size(); ++i) {
      const double mag = std::exp(6.0 * frand(seed) - 2.0);              // a wide dynamic range between bins
      Y[i] = (float)((frand(seed) * 2.0 - 1.0) * mag);
    }
    for (int o = 0; o < COUT; ++o)                                       // and between images: scales 1e-3 .. 1e4
      for (size_t q = 0; q < (size_t)NQ * NB; ++q)
        for (int e = 0; e < 8; ++e) Y[(q * COUT + o) * 8 + e] *= (float)std::pow(10.0, o - 3.0);
    // the largest magnitude: 2^13 (1 - 2^-24) is above anything the forward produces (|X| <= 60 * 80 values <= 1) and has the
    // mantissa of ones, the top of the interval the per-image scale maps to [2^13, 2^14).  d = Y[u] - Y[u + 32] = 2 Y[u] with
    // re = im (u % 16 < 8) or re = -im: at u = 8, 24 (cos = +-sin) a component of b is 2 sqrt(2) m, at u = 0 one of a is 0 and of b 2 m
    const float m = std::nextafterf(8192.0f, 0.0f);
    for (int v = 0; v < V; ++v)
      for (int u = 0; u < 32; ++u) {
        float* lo = &Y[spec_index(v * P + u, 0, NB, NQ, COUT, 0)];
        float* hi = &Y[spec_index(v * P + u + 32, 0, NB, NQ, COUT, 0)];
        lo[0] = (v & 1) ? -m : m;
        lo[1] = (u % 16 < 8) ? lo[0] : -lo[0];
        hi[0] = -lo[0];
        hi[1] = -lo[1];
      }
    std::vector<std::vector<double>> yref((size_t)NB * COUT);
    std::vector<double> ymaxo(COUT, 0.0);
    for (int nb = 0; nb < NB; ++nb)
      for (int o = 0; o < COUT; ++o) {
        inverse64(s, Y, nb, o, yref[(size_t)nb * COUT + o]);
        for (double v : yref[(size_t)nb * COUT + o]) ymaxo[o] = std::fmax(ymaxo[o], std::fabs(v));
      }
    std::vector<float> bp(3 * MTP, 0.f);
    for (int o = 0; o < COUT; ++o) {
      bp[o] = (float)(0.1 * (o - 3) * ymaxo[o]);
      bp[2 * MTP + o] = (float)std::ldexp(1.0, (int)std::floor(std::log2(4096.0 / (1.4 * ymaxo[o]))));
    }
    std::vector<double> got;
    const int flag = run_inverse(s, Y, bp, got);
    double worst = 0.0, worst_bound_image = 0.0;
    for (int nb = 0; nb < NB; ++nb)
      for (int o = 0; o < COUT; ++o)
        for (int i = 0; i < HW; ++i) {
          const double want = std::fmax(yref[(size_t)nb * COUT + o][i] + (double)bp[o], 0.0);
          const double e = std::fabs(got[((size_t)nb * COUT + o) * HW + i] - want) / ymaxo[o];
          worst = std::fmax(worst, e);
          if (nb == 0 && o == 0) worst_bound_image = std::fmax(worst_bound_image, e);
        }
    std::printf("inverse: max |y - float64| / max |y| = %.3e (the scale-bound image: %.3e), flag %d\n", worst, worst_bound_image, flag);
    if (!(worst <= 1.5e-6)) std::printf("INVERSE MISMATCH\n"), rc = 1;
    if (flag != 0) std::printf("RANGE FLAG RAISED\n"), rc = 1;
  }

  // ---------------- 3. round trip: the spectra of 1. (channel stride 8 = 8 output channels, channels 5 .. 7 zero) give x back
  {
    std::vector<float> bp(3 * MTP, 0.f);
    for (int o = 0; o < COUT; ++o) bp[2 * MTP + o] = 2048.0f;      // x < 1: activations below 2^11
    std::vector<double> got;
    const int flag = run_inverse(s, X, bp, got);
    double worst = 0.0;
    for (int nb = 0; nb < NB; ++nb)
      for (int o = 0; o < COUT; ++o)
        for (int i = 0; i < HW; ++i) {
          const double want = o < C ? x[((size_t)nb * C + o) * HW + i] : 0.0;
          worst = std::fmax(worst, std::fabs(got[((size_t)nb * COUT + o) * HW + i] - want));
        }
    const double bound = fwd_bound + 1.5e-6 * xmax;
    std::printf("round trip: max |x' - x| = %.3e (largest x %.3f, bound %.3e), flag %d\n", worst, xmax, bound, flag);
    if (!(worst <= bound) || flag != 0) std::printf("ROUND TRIP MISMATCH\n"), rc = 1;
  }
  std::printf(rc ? "FAILED\n" : "ok\n");
  return rc;
}
