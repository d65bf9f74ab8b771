// Host check of the planner of os2d_amd/csrc/dft_plan.h.  Built and run by tests/test_dft_plan_host.py.
// stdout: for both size policies (0: the smallest transform per map, 1: the canonical sizes), every map of the grid below and
// 4 and 8 images per iteration (dft_make_plan_policy, dft_plan_g8), one line - "none" or every field of the plan but the two
// magic numbers the launchers fill in (inv_cg, inv_og).  The test compares a digest of it with the one recorded from the planner
// before the LDS layout and the capacities were written once (profiles/dft_plan/README.md): the plans are the same plans.
//   the grid: H = 1 .. 100 x W = 1 .. 260; {2784, 2785} x {3600, 3601}; the seven levels of the benchmark pyramid
// stderr + exit status: the planner's own consistency - every LDS region of a plan ends inside what the plan budgets for it, the
// tail's contents inside the tail, the total inside the LDS of a work-group, and every count (tiles per product, window positions,
// spectrum items) within what the kernels declare.  -DDFT_PLAN_CHECK_PARENT compiles this part out and takes the planner from
// dft_mfma.h: the program then builds against a csrc/ from before dft_plan.h, with the same output.
#include <atomic>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#ifdef DFT_PLAN_CHECK_PARENT
#include "dft_emu.h"
#else
#include "dft_plan.h"      // on its own: the planner needs none of the kernels' hooks
#endif

using namespace os2d_dft;

static void line(std::string& out, int policy, int H, int W, int G, const DftPlan* p) {
  char buf[512];
  if (!p) {
    std::snprintf(buf, sizeof buf, "policy %d map %dx%d G %d: none\n", policy, H, W, G);
  } else {
    std::snprintf(buf, sizeof buf,
                  "policy %d map %dx%d G %d: H %d W %d P %d Q %d V %d NBINS %d T %d TY %d TX %d TH %d TW %d oy %d ox %d LH %d LW %d RH %d Pp %d "
                  "Wk %d N1 %d M2 %d Mx %d N2 %d MA %d MB %d KB %d NBo %d G %d eT %d fast %d inv_t %u inv_tx %u inv_c4 %u inv_v %u inv_pq %u "
                  "inv_kg %u inv_pp %u lds_const %d lds_union %d lds_total %d\n",
                  policy, H, W, G, p->H, p->W, p->P, p->Q, p->V, p->NBINS, p->T, p->TY, p->TX, p->TH, p->TW, p->oy, p->ox, p->LH, p->LW, p->RH,
                  p->Pp, p->Wk, p->N1, p->M2, p->Mx, p->N2, p->MA, p->MB, p->KB, p->NBo, p->G, p->eT, p->fast, p->inv_t, p->inv_tx, p->inv_c4,
                  p->inv_v, p->inv_pq, p->inv_kg, p->inv_pp, p->lds_const, p->lds_union, p->lds_total);
  }
  out += buf;
}

static std::atomic<long> n_checked{0}, n_failed{0};

static void consistent(int policy, const DftPlan& p) {
#ifndef DFT_PLAN_CHECK_PARENT
  const int G = p.G;
  const int rowop = G == 8 ? dft_lds_rowop(p.Pp, p.M2) * 16 : 0;
  const char* what = nullptr;
  if (dft_lds_fqt(p) * 16 + rowop > p.lds_const) what = "FqT (+ Fp2) ends behind lds_const";
  else if (dft_lds_gq(p) * 16 + rowop > p.lds_const) what = "Gq (+ E2) ends behind lds_const";
  else if (dft_lds_x_bytes(p) > p.lds_union) what = "x ends behind the union region";
  else if (dft_lds_n2_bytes(p) > p.lds_union) what = "R2 | Y2 ends behind the union region";
  else if (dft_lds_xs_bytes(p, G) > p.lds_union) what = "the X staging ends behind the union region";
  else if (dft_lds_tt_bytes(p) > p.lds_union) what = "Tt ends behind the union region";
  else if (dft_lds_tail(p) + DFT_TAIL_MAX + dft_tail_max_bytes(G) > p.lds_total) what = "the maxima end behind lds_total";
  else if (dft_lds_tail(p) + DFT_TAIL_TW + DFT_R2_TWU * 16 > p.lds_total) what = "the twiddles end behind lds_total";
  else if (dft_lds_tail(p) + DFT_TAIL_BYTES != p.lds_total) what = "lds_total is not the three regions";
  else if (p.lds_total > DFT_LDS_MAX) what = "lds_total is more than a work-group has";
  else if (!dft_capacity_ok(p)) what = "a count is beyond the kernels' capacity";
  else if (dft_ksteps_param(p) == DFT_R2_KS && !dft_radix2(p.P)) what = "8 k-steps without the 64-row transform";
  ++n_checked;
  if (what) {
    const DftCounts c = dft_plan_counts(p);
    if (n_failed++ < 20)
      std::fprintf(stderr, "INCONSISTENT policy %d map %dx%d G %d (P %d Q %d): %s; tiles %d %d %d %d, positions %d, items %d, lds %d + %d -> %d\n",
                   policy, p.H, p.W, G, p.P, p.Q, what, c.t1, c.t2, c.tA, c.tB, c.npos, c.nitem, p.lds_const, p.lds_union, p.lds_total);
  }
#else
  (void)policy, (void)p;
#endif
}

static void one_map(std::string& out, int policy, int H, int W) {
  DftPlan p4, p8;
  const bool ok4 = dft_make_plan_policy(H, W, policy, &p4);
  const bool ok8 = ok4 && dft_plan_g8(p4, &p8);
  line(out, policy, H, W, 4, ok4 ? &p4 : nullptr);
  line(out, policy, H, W, 8, ok8 ? &p8 : nullptr);
  if (ok4) consistent(policy, p4);
  if (ok8) consistent(policy, p8);
}

int main(int argc, char** argv) {
  constexpr int HMAX = 100, WMAX = 260;
  int nthreads = argc > 1 ? std::atoi(argv[1]) : (int)std::thread::hardware_concurrency();
  nthreads = nthreads < 1 ? 1 : nthreads > 16 ? 16 : nthreads;
  // rows of the grid are planned in parallel and printed in order
  std::vector<std::string> rows(2 * HMAX);
  std::atomic<int> next{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; ++t)
    pool.emplace_back([&] {
      for (int r = next++; r < 2 * HMAX; r = next++)
        for (int W = 1; W <= WMAX; ++W) one_map(rows[r], r / HMAX, r % HMAX + 1, W);
    });
  for (auto& th : pool) th.join();
  static const int LARGE[4][2] = {{2784, 3600}, {2784, 3601}, {2785, 3600}, {2785, 3601}};
  static const int PYRAMID[7][2] = {{30, 40}, {38, 50}, {48, 64}, {60, 80}, {72, 96}, {84, 112}, {96, 128}};
  for (int policy = 0; policy < 2; ++policy) {
    for (int h = 0; h < HMAX; ++h) std::fputs(rows[policy * HMAX + h].c_str(), stdout);
    std::string rest;
    for (auto& m : LARGE) one_map(rest, policy, m[0], m[1]);
    for (auto& m : PYRAMID) one_map(rest, policy, m[0], m[1]);
    std::fputs(rest.c_str(), stdout);
  }
#ifndef DFT_PLAN_CHECK_PARENT
  std::fprintf(stderr, "consistency: %ld plans checked, %ld failed\n", n_checked.load(), n_failed.load());
#endif
  return n_failed.load() ? 1 : 0;
}
