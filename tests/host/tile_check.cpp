// Host check of os2d_amd/csrc/tile_common.h - the strip-plane geometry and the XCD order the kernels compile, not a restatement:
//   every (tile, cell) of a launch is walked with os2d_conv_tiles / os2d_strip_origin / os2d_tile_cell: every data cell of the
//   map is produced by exactly one (tile, cell) with valid set, every pad cell of the data rows is owned exactly once and never
//   valid, nothing else is owned;
//   os2d_strip_cell of every slab index a tile loads is 0 or a data cell of the plane, and - in the slab's interior - the cell
//   whose row and column the way back (os2d_tile_cell) names;
//   os2d_xcd_logical is a permutation of the grid.
// `tile_check dump H W R HALO_ROUND FILE` writes os2d_strip_cell of every slab index of every tile as int32 (what
// tests/test_tile_host.py compares with the numpy model of tests/test_conv_strips_model.py).  Built and run by tests/test_tile_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#define OS2D_HOST_EMU 1
#include "tile_common.h"

static int round_up(int x, int m) { return (x + m - 1) / m * m; }
static int os2d_ws(int W) { return W + OS2D_PAD; }
static int base(int W) { return round_up(OS2D_PAD * os2d_ws(W) + OS2D_PAD, 4); }                             // os2d_base
static int plane(int H, int W) { return round_up(base(W) + (H + OS2D_PAD) * os2d_ws(W) + OS2D_PAD, 64); }    // os2d_plane

constexpr int NT = 256;
static int failures = 0;
#define CHECK(c, ...)                       \
  if (!(c)) {                               \
    if (++failures <= 20) {                 \
      printf("FAILED %s: ", #c);            \
      printf(__VA_ARGS__);                  \
      printf("\n");                         \
    }                                       \
  }

// one launch: strip = the kernels' choice for this width (or forced), halo_round = 1 (conv_f16x3, conv3_f16x3) | 4 (conv_mfma)
static void walk(int H, int W, int R, bool strip, int halo_round, FILE* dump) {
  const int Ws = os2d_ws(W), BASE = base(W), PLANE = plane(H, W);
  int SP, TPS;
  const int tiles = os2d_conv_tiles(strip, H, W, R, NT, &SP, &TPS);
  CHECK(strip ? (SP > 2 * R && TPS > 0 && tiles % TPS == 0) : (SP == 0 && TPS == 0), "H=%d W=%d R=%d", H, W, R);
  const int PW = strip ? SP : Ws, HALO = round_up(R * PW + R, halo_round);
  std::vector<int> owned(PLANE, 0), valid(PLANE, 0);
  for (int tile = 0; tile < tiles; ++tile) {
    const int s = strip ? tile / TPS : 0;
    const int c0mR = strip ? os2d_strip_origin(s, SP, R) : 0;
    const int n0 = strip ? (tile - s * TPS) * NT : BASE + tile * NT;
    for (int p = 0; p < NT; ++p) {
      int hr, wc, cell;
      bool v;
      if (!os2d_tile_cell(strip, n0 + p, SP, R, c0mR, H, W, Ws, BASE, PLANE, &hr, &wc, &cell, &v)) continue;
      CHECK(cell >= 0 && cell < PLANE, "cell %d of tile %d outside the plane (H=%d W=%d R=%d)", cell, tile, H, W, R);
      if (cell < 0 || cell >= PLANE) continue;
      ++owned[cell];
      if (v) {
        ++valid[cell];
        CHECK(cell == BASE + hr * Ws + wc && hr >= 0 && hr < H && wc >= 0 && wc < W, "valid cell %d = (%d, %d) (H=%d W=%d)", cell, hr, wc, H, W);
      }
      if (strip && v) {       // the slab cell under the centre tap is this very cell, its neighbours are its neighbours or zero
        for (int dy = -R; dy <= R; ++dy)
          for (int dx = -R; dx <= R; ++dx) {
            const int got = os2d_strip_cell(n0 + p + dy * SP + dx, SP, c0mR, H, W, Ws, BASE);
            const bool in = hr + dy >= 0 && hr + dy < H && wc + dx >= 0 && wc + dx < W;
            CHECK(got == (in ? BASE + (hr + dy) * Ws + wc + dx : 0), "tap (%d, %d) of cell (%d, %d): %d (H=%d W=%d R=%d)", dy, dx, hr, wc, got, H, W, R);
          }
      }
    }
    if (strip)
      for (int i = 0; i < NT + 2 * HALO; ++i) {
        const int c = os2d_strip_cell(n0 - HALO + i, SP, c0mR, H, W, Ws, BASE);
        const int r = c - BASE;
        CHECK(c == 0 || (r >= 0 && r / Ws < H && r % Ws < W), "slab unit %d of tile %d -> %d: not a data cell (H=%d W=%d R=%d)", i, tile, c, H, W, R);
        if (dump) fwrite(&c, sizeof(int), 1, dump);
      }
  }
  for (int c = 0; c < PLANE; ++c) {
    const int r = c - BASE;
    const bool row = r >= 0 && r < H * Ws, data = row && r % Ws < W;
    // linear tiles run to the end of the last tile: what they own past the data rows is pad (the kernels store zeros there)
    const int want_owned = row ? 1 : (!strip && r >= 0 && r < tiles * NT ? 1 : 0);
    CHECK(owned[c] == want_owned && valid[c] == (data ? 1 : 0), "cell %d: owned %d (want %d), valid %d, data %d (H=%d W=%d R=%d strip=%d)", c, owned[c],
          want_owned, valid[c], (int)data, H, W, R, (int)strip);
  }
}

int main(int argc, char** argv) {
  if (argc == 7 && argv[1][0] == 'd') {
    FILE* f = fopen(argv[6], "wb");
    if (!f) return 2;
    walk(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), true, atoi(argv[5]), f);
    fclose(f);
    return failures ? 1 : 0;
  }
  const int widths[] = {1, 80, 209, 316, 317, 509, 510, 1000, 3600}, heights[] = {1, 2, 7, 33};
  int launches = 0;
  for (int R = 2; R <= 3; ++R)
    for (int W : widths)
      for (int H : heights)
        for (int halo_round : {1, 4}) {
          walk(H, W, R, W > 316, halo_round, nullptr);      // what the kernels launch (OS2D_MAX_W_LINEAR5 = 316)
          ++launches;
        }
  // the strip count changes between W = 509 and 510: Ws 512 -> 513
  int NS, SP;
  os2d_conv_strips(509, 2, &NS, &SP);
  CHECK(NS == 2 && SP == 260, "W=509: NS %d SP %d", NS, SP);
  os2d_conv_strips(510, 2, &NS, &SP);
  CHECK(NS == 3 && SP == 175, "W=510: NS %d SP %d", NS, SP);
  for (unsigned grid : {8u, 16u, 40u, 1288u}) {
    std::vector<int> seen(grid, 0);
    for (unsigned b = 0; b < grid; ++b) {
      const int l = os2d_xcd_logical(b, grid);
      CHECK(l >= 0 && l < (int)grid && l / (int)(grid / 8) == (int)(b % 8), "xcd order: block %u of %u -> %d", b, grid, l);
      if (l >= 0 && l < (int)grid) ++seen[l];
    }
    for (unsigned l = 0; l < grid; ++l) CHECK(seen[l] == 1, "xcd order: logical %u of %u taken %d times", l, grid, seen[l]);
  }
  printf("tile geometry: %d launches, %d failed checks\n%s\n", launches, failures, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
