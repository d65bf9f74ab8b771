// Host check of os2d_amd/csrc/dft_mfma.h on the SPMD emulator (spmd_emu.h): the forward and the inverse transform kernels -
// the same source the GPU runs - against float64 DFTs, for an untiled fast-path map, a map whose width is not a multiple of 4,
// a small map and tiled maps (ragged tiles).  Built and run by tests/test_dft_mfma_host.py.   usage: dft_mfma_check [H W C NB]...
#include "dft_emu.h"      // the hooks on the emulator (policy 0: the smallest transform per map), dft_mfma.h, spec_index, table, frand, ws_of / base_of / plane_of

using namespace os2d_dft;

static int check_case(int H, int W, int C, int NB, int grid) {
  DftPlan pl;
  if (!dft_make_plan(H, W, &pl)) {
    std::printf("no plan for %dx%d\n", H, W);
    return 1;
  }
  const int P = pl.P, Q = pl.Q, V = pl.V, T = pl.T, NBT = NB * T, Cpad = dft_round_up(C, 8) + 0, HW = H * W;
  std::printf("case %dx%d C=%d NB=%d: P=%d Q=%d bins=%d tiles=%dx%d (%dx%d) window %dx%d lds=%d fast=%d\n", H, W, C, NB, P, Q, pl.NBINS,
              pl.TY, pl.TX, pl.TH, pl.TW, pl.LH, pl.LW, pl.lds_total, pl.fast);
  const std::vector<double> tp = table(P), tq = table(Q);
  std::vector<u32x4> mats(dft_matrices_units(P, Q));
  const int nf = dft_units_fqt(P, Q), n2 = dft_units_fp2(P, Q), ne = dft_units_e2(P, Q), ng = dft_units_gq(P, Q);
  for (int i = 0; i < nf; ++i) dft_matrix_unit(0, i, P, Q, tp.data(), tq.data(), &mats[i]);
  for (int i = 0; i < n2; ++i) dft_matrix_unit(1, i, P, Q, tp.data(), tq.data(), &mats[nf + i]);
  for (int i = 0; i < ne; ++i) dft_matrix_unit(2, i, P, Q, tp.data(), tq.data(), &mats[nf + n2 + i]);
  for (int i = 0; i < ng; ++i) dft_matrix_unit(3, i, P, Q, tp.data(), tq.data(), &mats[nf + n2 + ne + i]);
  const u32x4 *FqT = mats.data(), *Fp2 = FqT + nf, *E2 = Fp2 + n2, *Gq = E2 + ne;

  // ---------------- forward
  unsigned seed = 12345u + H * 131 + W;
  std::vector<float> corr((size_t)NB * C * HW), invn((size_t)NB * HW);
  for (auto& v : corr) v = (float)(frand(seed) * 2.0 - 0.7);
  for (auto& v : invn) v = (float)(0.2 + 0.5 * frand(seed));          // relu(corr) * invn <= 1.3 * 0.7 < 1
  std::vector<float> X((size_t)(pl.NBINS / 4) * NBT * Cpad * 8, 777.0f);
  // both shapes of the kernels: 4 images per iteration (row operand of step 2 / step A in registers), and - where the transform takes
  // it - 8 images (row operand in LDS, whole activation units)
  DftPlan pl8;
  const bool have8 = dft_plan_g8(pl, &pl8) && Cpad % 8 == 0;
  if (!have8) std::printf("  (no 8-image plan for this transform)\n");
  for (int G = 4; G <= 8; G += 4) {
    if (G == 8 && !have8) continue;
    DftPlan fp = G == 8 ? pl8 : pl;
    const int CGf = (C + G - 1) / G, itf = NBT * CGf;
    fp.inv_cg = dft_magic((unsigned)CGf);
    std::fill(X.begin(), X.end(), 777.0f);
    emu::launch(grid, 512, fp.lds_total, [&] {
      if (G == 4) {
        // the instantiation dft_ksteps_param chooses for the plan, as dft_forward_pick of the device build (dft_mfma.hip)
#define FWD4(KS)                                                                                                             \
  if (fp.T > 1) dft_forward_body<true, false, 4, 8, KS>(corr.data(), invn.data(), X.data(), FqT, Fp2, fp, C, Cpad, NBT, itf);  \
  else if (fp.fast) dft_forward_body<false, true, 4, 8, KS>(corr.data(), invn.data(), X.data(), FqT, Fp2, fp, C, Cpad, NBT, itf); \
  else dft_forward_body<false, false, 4, 8, KS>(corr.data(), invn.data(), X.data(), FqT, Fp2, fp, C, Cpad, NBT, itf);
        switch (dft_ksteps_param(fp)) {
          case 5: FWD4(5) break;
          case 6: FWD4(6) break;
          case 7: FWD4(7) break;
          case 8: FWD4(8) break;
          default: FWD4(0) break;
        }
#undef FWD4
      } else {
        if (fp.T > 1) dft_forward_body<true, false, 8, 8>(corr.data(), invn.data(), X.data(), FqT, Fp2, fp, C, Cpad, NBT, itf);
        else if (fp.fast) dft_forward_body<false, true, 8, 8>(corr.data(), invn.data(), X.data(), FqT, Fp2, fp, C, Cpad, NBT, itf);
        else dft_forward_body<false, false, 8, 8>(corr.data(), invn.data(), X.data(), FqT, Fp2, fp, C, Cpad, NBT, itf);
      }
    });
  double worst = 0.0, scale = 0.0;
  for (int nb = 0; nb < NB; ++nb)
    for (int tile = 0; tile < T; ++tile) {
      const int ty = tile / pl.TX, tx = tile % pl.TX;
      const int Y0 = T > 1 ? ty * pl.TH - pl.oy : 0, X0 = T > 1 ? tx * pl.TW - pl.ox : 0;
      for (int c = 0; c < C; ++c) {
        std::vector<double> x((size_t)pl.LH * pl.LW, 0.0);
        for (int r = 0; r < pl.LH; ++r)
          for (int cc = 0; cc < pl.LW; ++cc) {
            const int y = Y0 + r, xx = X0 + cc;
            if (y >= 0 && y < H && xx >= 0 && xx < W) {
              const float a = corr[((size_t)nb * C + c) * HW + y * W + xx], n = invn[(size_t)nb * HW + y * W + xx];
              x[(size_t)r * pl.LW + cc] = (double)(std::fmax(a, 0.f) * n);
            }
          }
        // row transforms then column transforms in float64
        std::vector<double> rr((size_t)pl.LH * V), ri((size_t)pl.LH * V);
        for (int r = 0; r < pl.LH; ++r)
          for (int v = 0; v < V; ++v) {
            double sr = 0, si = 0;
            for (int cc = 0; cc < pl.LW; ++cc) {
              const int a = (int)(((long long)v * cc) % Q);
              sr += x[(size_t)r * pl.LW + cc] * tq[2 * a];
              si += x[(size_t)r * pl.LW + cc] * tq[2 * a + 1];
            }
            rr[(size_t)r * V + v] = sr;
            ri[(size_t)r * V + v] = si;
          }
        const int pair = nb * T + tile;
        for (int u = 0; u < P; ++u)
          for (int v = 0; v < V; ++v) {
            double sr = 0, si = 0;
            for (int r = 0; r < pl.LH; ++r) {
              const int a = (int)(((long long)u * r) % P);
              const double cr = tp[2 * a], ci = tp[2 * a + 1];
              sr += rr[(size_t)r * V + v] * cr - ri[(size_t)r * V + v] * ci;
              si += rr[(size_t)r * V + v] * ci + ri[(size_t)r * V + v] * cr;
            }
            const int bin = v * P + u;
            const float* got = &X[spec_index(bin, pair, NBT, pl.NBINS / 4, Cpad, c)];
            worst = std::fmax(worst, std::fmax(std::fabs(got[0] - sr), std::fabs(got[1] - si)));
            scale = std::fmax(scale, std::fmax(std::fabs(sr), std::fabs(si)));
          }
        for (int bin = P * V; bin < pl.NBINS; ++bin) {
          const float* got = &X[spec_index(bin, pair, NBT, pl.NBINS / 4, Cpad, c)];
          if (got[0] != 0.f || got[1] != 0.f) {
            std::printf("padding bin %d not zero\n", bin);
            return 1;
          }
        }
      }
    }
  std::printf("  forward (G = %d): max |X - float64| = %.3e (largest |X| %.1f)\n", G, worst, scale);
  if (!(worst <= 2e-6 * scale + 1e-5)) {
    std::printf("FORWARD MISMATCH\n");
    return 1;
  }
  }

  // ---------------- inverse (Cout = 16 output channels: 4 / 2 groups)
  const int Cout = 16, MTP = 128, PLANE = plane_of(H, W), Ws = ws_of(W), BASE = base_of(W);
  std::vector<float> Y((size_t)(pl.NBINS / 4) * NBT * Cout * 8);
  for (size_t i = 0; i < Y.size(); ++i) {
    const double mag = std::exp(6.0 * frand(seed) - 2.0);              // a wide dynamic range between bins
    Y[i] = (float)((frand(seed) * 2.0 - 1.0) * mag);
  }
  for (int o = 0; o < Cout; ++o)                                       // and between images: scales 1e-3 .. 1e4
    for (size_t q = 0; q < (size_t)(pl.NBINS / 4) * NBT; ++q)
      for (int e = 0; e < 8; ++e) Y[(q * Cout + o) * 8 + e] *= (float)std::pow(10.0, (o % 8) - 3.0);
  // float64 inverse first: the channel scales of the epilogue are chosen from it the way the range plan does for the real
  // network (activations a few binades below 2^15: both fp16 halves normal)
  std::vector<double> yref((size_t)NB * Cout * HW, 0.0), ymaxo(Cout, 0.0);
  for (int nb = 0; nb < NB; ++nb)
    for (int o = 0; o < Cout; ++o)
      for (int tile = 0; tile < T; ++tile) {
        const int ty = tile / pl.TX, tx = tile % pl.TX, pair = nb * T + tile;
        const int y0 = T > 1 ? ty * pl.TH : 0, x0 = T > 1 ? tx * pl.TW : 0;
        const int TH_ = T > 1 ? pl.TH : H, TW_ = T > 1 ? pl.TW : W;
        for (int th = 0; th < TH_ && y0 + th < H; ++th) {
          const int hwin = th + pl.oy;
          std::vector<double> tr(V), ti(V);
          for (int v = 0; v < V; ++v) {
            double sr = 0, si = 0;
            for (int u = 0; u < P; ++u) {
              const int bin = v * P + u;
              const float* y = &Y[spec_index(bin, pair, NBT, pl.NBINS / 4, Cout, o)];
              const int a = (int)(((long long)u * hwin) % P);
              const double cr = tp[2 * a], ci = -tp[2 * a + 1];      // e^{+i}
              sr += y[0] * cr - y[1] * ci;
              si += y[0] * ci + y[1] * cr;
            }
            tr[v] = sr;
            ti[v] = si;
          }
          for (int tw = 0; tw < TW_ && x0 + tw < W; ++tw) {
            const int wwin = tw + pl.ox;
            double s2 = 0;
            for (int v = 0; v < V; ++v) {
              const double a_v = (v == 0 || 2 * v == Q) ? 1.0 : 2.0;
              const int a = (int)(((long long)v * wwin) % Q);
              s2 += a_v * (tr[v] * tq[2 * a] + ti[v] * tq[2 * a + 1]);     // Re(T e^{+i theta}) = Tr cos - Ti sin; tq = (cos, -sin)
            }
            const double yv = s2 / ((double)P * Q);
            yref[((size_t)nb * Cout + o) * HW + (size_t)(y0 + th) * W + x0 + tw] = yv;
            ymaxo[o] = std::fmax(ymaxo[o], std::fabs(yv));
          }
        }
      }
  std::vector<float> bp(3 * MTP, 0.f);
  for (int o = 0; o < Cout; ++o) {
    bp[o] = (float)(0.1 * ((o % 8) - 3) * ymaxo[o]);
    bp[2 * MTP + o] = (float)std::ldexp(1.0, (int)std::floor(std::log2(4096.0 / (1.4 * ymaxo[o]))));
  }
  for (int G = 4; G <= 8; G += 4) {
  if (G == 8 && !have8) continue;
  DftPlan ip = G == 8 ? pl8 : pl;
  std::vector<unsigned char> out((size_t)NB * ((Cout + 7) / 8) * 2 * PLANE * 16, 0x5A);     // a pattern: the kernel writes the borders too
  int flag = 0;
  const int OG = Cout / G, iters_i = NBT * OG;
  ip.inv_og = dft_magic((unsigned)OG);
  emu::launch(grid, DFT_THR, ip.lds_total, [&] {
#define INV(KS)                                                                                                                     \
  if (ip.T > 1) dft_inverse_body<true, KS>(Y.data(), bp.data(), MTP, out.data(), E2, Gq, ip, Cout, NBT, PLANE, Ws, BASE, iters_i, &flag, 1); \
  else dft_inverse_body<false, KS>(Y.data(), bp.data(), MTP, out.data(), E2, Gq, ip, Cout, NBT, PLANE, Ws, BASE, iters_i, &flag, 1);
    if (G == 8) {
      if (ip.T > 1) dft_inverse_body<true, 0, 8>(Y.data(), bp.data(), MTP, out.data(), E2, Gq, ip, Cout, NBT, PLANE, Ws, BASE, iters_i, &flag, 1);
      else dft_inverse_body<false, 0, 8>(Y.data(), bp.data(), MTP, out.data(), E2, Gq, ip, Cout, NBT, PLANE, Ws, BASE, iters_i, &flag, 1);
    } else
    switch (dft_ksteps_param(ip)) {      // as dft_inverse_pick of the device build
      case 5: INV(5) break;
      case 6: INV(6) break;
      case 7: INV(7) break;
      case 8: INV(8) break;
      default: INV(0) break;
    }
#undef INV
  });
  double worst_rel = 0.0;
  for (int nb = 0; nb < NB; ++nb)
    for (int o = 0; o < Cout; ++o) {
      const unsigned char* hi = &out[(((size_t)nb * ((Cout + 7) / 8) + (o >> 3)) * 2 + 0) * (size_t)PLANE * 16];
      const unsigned char* lo = &out[(((size_t)nb * ((Cout + 7) / 8) + (o >> 3)) * 2 + 1) * (size_t)PLANE * 16];
      const double unit = ymaxo[o] * (double)bp[2 * MTP + o];
      for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w) {
          const size_t cell = (size_t)BASE + (size_t)h * Ws + w;
          const _Float16 hv = *reinterpret_cast<const _Float16*>(hi + cell * 16 + (o & 7) * 2);
          const _Float16 lv = *reinterpret_cast<const _Float16*>(lo + cell * 16 + (o & 7) * 2);
          const double want = std::fmax(yref[((size_t)nb * Cout + o) * HW + (size_t)h * W + w] + (double)bp[o], 0.0) * (double)bp[2 * MTP + o];
          worst_rel = std::fmax(worst_rel, std::fabs((double)hv + (double)lv - want) / unit);
        }
    }
  // the kernel also writes the zero borders of the planes (the buffer was filled with a pattern)
  for (int nb = 0; nb < NB; ++nb)
    for (int pln = 0; pln < ((Cout + 7) / 8) * 2; ++pln) {
      const unsigned char* base = &out[((size_t)nb * ((Cout + 7) / 8) * 2 + pln) * (size_t)PLANE * 16];
      for (int cell = 0; cell < PLANE; ++cell) {
        const int rel = cell - BASE, hh = rel >= 0 ? rel / Ws : -1, ww = rel >= 0 ? rel % Ws : -1;
        if (rel >= 0 && hh < H && ww < W) continue;
        for (int b = 0; b < 16; ++b)
          if (base[(size_t)cell * 16 + b] != 0) {
            std::printf("border cell %d of plane %d (pair %d) not zero\n", cell, pln, nb);
            return 1;
          }
      }
    }
  std::printf("  inverse (G = %d): max |y - float64| / max |y| = %.3e, flag %d\n", G, worst_rel, flag);
  if (!(worst_rel <= 1.5e-6) || flag != 0) {
    std::printf("INVERSE MISMATCH\n");
    return 1;
  }
  }
  return 0;
}

// ---------------- the range flag of the inverse transform (usage: dft_mfma_check range H W NB ...)
// Every (pair, channel) holds the spectrum of a scaled delta image, Y[u][v] = A exp(-2 pi i (u hwin / P + v wwin / Q)): the
// inverse transform gives A at window cell (hwin, wwin) and 0 elsewhere, and with bias 0 and scale 1 the stored value IS A.
// LOW = 65504 (1 - 2^-10) everywhere is the clean twin; the cases then change ONE spectrum of the LAST pair (its last tile):
//   over      A = 65504 (1 + 2^-10) at the map's last cell                                       -> flag
//   nan       one bin of that spectrum is NaN and the channel's bias is -1: every pre-activation
//             of the channel is NaN and fmaxf(NaN, 0) = 0 stores a clean 0                       -> flag
//   overhang  A = 65504 (1 + 2^-10) at a window cell the kernel does not store (below the map /
//             in the halo of a tiled transform: inside == false)                                 -> no flag
// 2^-10 is ~650 times the 1.5e-6 this file holds the inverse transform to.
static int check_range_flag(int H, int W, int NB, int grid) {
  DftPlan pl;
  if (!dft_make_plan(H, W, &pl)) {
    std::printf("no plan for %dx%d\n", H, W);
    return 1;
  }
  const int P = pl.P, Q = pl.Q, V = pl.V, T = pl.T, NBT = NB * T;
  const std::vector<double> tp = table(P), tq = table(Q);
  std::vector<u32x4> mats(dft_matrices_units(P, Q));
  const int nf = dft_units_fqt(P, Q), n2 = dft_units_fp2(P, Q), ne = dft_units_e2(P, Q), ng = dft_units_gq(P, Q);
  for (int i = 0; i < nf; ++i) dft_matrix_unit(0, i, P, Q, tp.data(), tq.data(), &mats[i]);
  for (int i = 0; i < n2; ++i) dft_matrix_unit(1, i, P, Q, tp.data(), tq.data(), &mats[nf + i]);
  for (int i = 0; i < ne; ++i) dft_matrix_unit(2, i, P, Q, tp.data(), tq.data(), &mats[nf + n2 + i]);
  for (int i = 0; i < ng; ++i) dft_matrix_unit(3, i, P, Q, tp.data(), tq.data(), &mats[nf + n2 + ne + i]);
  const u32x4 *E2 = mats.data() + nf + n2, *Gq = E2 + ne;
  DftPlan pl8;
  const bool have8 = dft_plan_g8(pl, &pl8);
  const int Cout = 16, MTP = 128, PLANE = plane_of(H, W), Ws = ws_of(W), BASE = base_of(W);
  const double LOW = 65504.0 * (1.0 - 1.0 / 1024.0), HIGH = 65504.0 * (1.0 + 1.0 / 1024.0);
  // window cell of map cell (h, w) in the last tile, and a window cell of that tile which is not stored
  const int ty = pl.TY - 1, tx = pl.TX - 1, y0 = T > 1 ? ty * pl.TH : 0, x0 = T > 1 ? tx * pl.TW : 0;
  const int oy = T > 1 ? pl.oy : 0, ox = T > 1 ? pl.ox : 0;
  const int last_h = H - 1 - y0 + oy, last_w = W - 1 - x0 + ox;
  const int out_h = T > 1 ? 0 : H, out_w = T > 1 ? 0 : W - 1;        // tiled: the halo corner; untiled: the row below the map
  if (!(T > 1 ? (oy > 0 || ox > 0) : H < P)) {
    std::printf("no unstored window cell for %dx%d\n", H, W);
    return 1;
  }
  const int bad_pair = NBT - 1, bad_o = Cout - 3;
  struct Case { const char* name; double amp; int hwin, wwin; bool nan; int want; };
  const Case cases[] = {{"clean", LOW, last_h, last_w, false, 0}, {"over", HIGH, last_h, last_w, false, 1},
                        {"nan", LOW, last_h, last_w, true, 1}, {"overhang", HIGH, out_h, out_w, false, 0}};
  for (const Case& cs : cases)
    for (int G = 4; G <= 8; G += 4) {
      if (G == 8 && !have8) continue;
      std::vector<float> Y((size_t)(pl.NBINS / 4) * NBT * Cout * 8, 0.f);
      for (int pair = 0; pair < NBT; ++pair)
        for (int o = 0; o < Cout; ++o) {
          const bool it = pair == bad_pair && o == bad_o;
          const double A = it ? cs.amp : LOW;
          // the others sit at the first cell of their tile (window cell (oy, ox): inside for every tile)
          const int hwin = it ? cs.hwin : oy, wwin = it ? cs.wwin : ox;
          for (int u = 0; u < P; ++u)
            for (int v = 0; v < V; ++v) {
              const int a = (int)(((long long)u * hwin) % P), b = (int)(((long long)v * wwin) % Q);
              float* y = &Y[spec_index(v * P + u, pair, NBT, pl.NBINS / 4, Cout, o)];
              y[0] = (float)(A * (tp[2 * a] * tq[2 * b] - tp[2 * a + 1] * tq[2 * b + 1]));
              y[1] = (float)(A * (tp[2 * a] * tq[2 * b + 1] + tp[2 * a + 1] * tq[2 * b]));
            }
        }
      std::vector<float> bp(3 * MTP, 0.f);
      for (int o = 0; o < Cout; ++o) bp[2 * MTP + o] = 1.f;
      if (cs.nan) {
        Y[spec_index(1 * P + 2, bad_pair, NBT, pl.NBINS / 4, Cout, bad_o)] = std::nanf("");
        bp[bad_o] = -1.f;
      }
      DftPlan ip = G == 8 ? pl8 : pl;
      std::vector<unsigned char> out((size_t)NB * ((Cout + 7) / 8) * 2 * PLANE * 16, 0x5A);
      int flag = 0;
      const int OG = Cout / G, iters_i = NBT * OG;
      ip.inv_og = dft_magic((unsigned)OG);
      emu::launch(grid, DFT_THR, ip.lds_total, [&] {
#define INV(KS)                                                                                                                     \
  if (ip.T > 1) dft_inverse_body<true, KS>(Y.data(), bp.data(), MTP, out.data(), E2, Gq, ip, Cout, NBT, PLANE, Ws, BASE, iters_i, &flag, 1); \
  else dft_inverse_body<false, KS>(Y.data(), bp.data(), MTP, out.data(), E2, Gq, ip, Cout, NBT, PLANE, Ws, BASE, iters_i, &flag, 1);
        if (G == 8) {
          if (ip.T > 1) dft_inverse_body<true, 0, 8>(Y.data(), bp.data(), MTP, out.data(), E2, Gq, ip, Cout, NBT, PLANE, Ws, BASE, iters_i, &flag, 1);
          else dft_inverse_body<false, 0, 8>(Y.data(), bp.data(), MTP, out.data(), E2, Gq, ip, Cout, NBT, PLANE, Ws, BASE, iters_i, &flag, 1);
        } else
          switch (dft_ksteps_param(ip)) {
            case 5: INV(5) break;
            case 6: INV(6) break;
            case 7: INV(7) break;
            case 8: INV(8) break;
            default: INV(0) break;
          }
#undef INV
      });
      // the value the case is about, as stored (the map's last cell of the changed channel), and the largest other value
      const int nb = NB - 1;
      const size_t cell = (size_t)BASE + (size_t)(H - 1) * Ws + (W - 1);
      const unsigned char* hi = &out[(((size_t)nb * ((Cout + 7) / 8) + (bad_o >> 3)) * 2 + 0) * (size_t)PLANE * 16];
      const unsigned char* lo = &out[(((size_t)nb * ((Cout + 7) / 8) + (bad_o >> 3)) * 2 + 1) * (size_t)PLANE * 16];
      const float hv = (float)*reinterpret_cast<const _Float16*>(hi + cell * 16 + (bad_o & 7) * 2);
      const float lv = (float)*reinterpret_cast<const _Float16*>(lo + cell * 16 + (bad_o & 7) * 2);
      std::printf("  range %dx%d %-8s (G = %d): flag %d (want %d), stored hi %g lo %g\n", H, W, cs.name, G, flag, cs.want, hv, lv);
      if (flag != cs.want) {
        std::printf("RANGE FLAG MISMATCH\n");
        return 1;
      }
      // the clean twin and the overhang case store finite values only; the stored cell of the clean twin is LOW to 1.5e-6
      if (cs.want == 0 && cs.hwin == last_h && !(std::fabs((double)hv + (double)lv - LOW) <= 1.5e-6 * LOW)) {
        std::printf("RANGE TWIN VALUE MISMATCH\n");
        return 1;
      }
    }
  return 0;
}

int main(int argc, char** argv) {
  int rc = 0;
  if (argc >= 2 && argv[1][0] == 'r') {      // "range" as the first argument: the range flag cases, H W NB per map
    for (int i = 2; i + 2 < argc; i += 3) rc |= check_range_flag(std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), 2);
    std::printf(rc ? "FAILED\n" : "ok\n");
    return rc;
  }
  if (argc >= 2 && argv[1][0] == 'c') {      // "canonical" as the first argument: plan on the six canonical transform sizes
    emu_dft_policy = 1;
    --argc;
    ++argv;
  }
  if (argc >= 5) {
    for (int i = 1; i + 3 < argc; i += 4) rc |= check_case(std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]), 2);
  } else {
    rc |= check_case(11, 13, 5, 1, 2);       // small, W % 4 != 0, a partial channel group
    rc |= check_case(20, 24, 4, 2, 3);       // fast path, two pairs, more work-groups than one iteration each
  }
  std::printf(rc ? "FAILED\n" : "ok\n");
  return rc;
}
