// k2_walk_host.cpp -- K2's chroma walk (lives_amd/csrc/k2_walk.h) on the CPU: the header's accessor forms with plain integer arithmetic, no HIP anywhere.
// tests/test_k2_walk_cpu.py builds this with the address and undefined-behaviour sanitizers, runs it as a child process and compares every byte it writes with
// the oracle's orc_yuv420p_to_rgb.  Every plane is allocated at exactly its stated size, so the walk's read one past a plane's end must be clamped to pass.
//
//   k2_walk_host IN OUT
// IN (int32, little endian): four table sets [4][5][256] (RGB_Y R_Cr G_Cb G_Cr B_Cb), the number of cases, then per case
//   w h is_422 ys us vs ysize usize vsize which_tables low_quality fix_edges, and the three planes.
// OUT: per case h rows of w RGBA pixels.
#include "k2_walk.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace lgpu;

static int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
static int clamp16_240(int n) {      // CLAMP16_240
  if (n < 0) return 16;
  if (n > 255 || (n & 0xF0) == 0xF0) return 240;
  return (n & 0xF0) ? n : 16;
}

struct Case { int32_t w, h, is422, ys, us, vs, ysize, usize, vsize, which, lowq, fix; };

static bool get(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: k2_walk_host IN OUT\n"); return 2; }
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
  std::vector<int32_t> tables(4 * 5 * 256);
  int32_t ncases = 0;
  if (!get(in, tables.data(), tables.size() * 4) || !get(in, &ncases, 4)) { fprintf(stderr, "short input\n"); return 2; }
  for (int n = 0; n < ncases; n++) {
    Case c;
    if (!get(in, &c, sizeof c)) { fprintf(stderr, "short case %d\n", n); return 2; }
    // exactly the stated sizes: one byte past a plane is the sanitizer's
    uint8_t *Y = (uint8_t *)malloc(c.ysize), *U = (uint8_t *)malloc(c.usize), *V = (uint8_t *)malloc(c.vsize);
    if (!get(in, Y, c.ysize) || !get(in, U, c.usize) || !get(in, V, c.vsize)) { fprintf(stderr, "short planes %d\n", n); return 2; }
    const int32_t *ty = &tables[c.which * 1280], *rcr = ty + 256, *gcb = ty + 512, *gcr = ty + 768, *bcb = ty + 1024;
    const bool clamped = !(c.which & 1);
    const int w = c.w, h = c.h, hw = w >> 1;
    std::vector<uint32_t> dst((size_t)w * h, 0u);
    auto PU = [&](int r, int k) -> int { const long i = (long)r * c.us + k; return U[i < c.usize ? i : c.usize - 1]; };
    auto PV = [&](int r, int k) -> int { const long i = (long)r * c.vs + k; return V[i < c.vsize ? i : c.vsize - 1]; };
    auto cuv = [&](int v) -> int { return clamped ? clamp16_240(v) : clamp255(v); };
    auto px = [&](int y, int iu, int iv) -> uint32_t {
      const int u = cuv(iu), v = cuv(iv);
      const uint32_t r = clamp255((ty[y] + rcr[v]) >> 16), g = clamp255((ty[y] + gcb[u] + gcr[v]) >> 16), b = clamp255((ty[y] + bcb[u]) >> 16);
      return r | (g << 8) | (b << 16) | 0xFF000000u;
    };
    auto blend = [&](int s1, int s2, int &top, int &bot) {
      if (c.lowq) { top = s1 >> 1; bot = s2 >> 1; }
      else { top = (s1 + (s2 >> 1) + 1) / 3; bot = ((s1 >> 1) + s2 + 1) / 3; }
    };
    auto yat = [&](int row, int x) -> int { return Y[(size_t)row * c.ys + x]; };
    for (int k = 0; k < hw; k++) {
      uint32_t *d = dst.data() + 2 * k;
      if (c.is422) {
        for (int i = 0; i < h; i++) k2_row_pixels(k2_row_422(i, k, PU, PV), yat(i, 2 * k), yat(i, 2 * k + 1), px, d[(size_t)i * w], d[(size_t)i * w + 1]);
        continue;
      }
      k2_row_pixels(k2_row_edge(0, k, hw, PU, PV), yat(0, 2 * k), yat(0, 2 * k + 1), px, d[0], d[1]);
      const int npairs = (h - 1) / 2;
      for (int p = 1; p <= npairs; p++) {
        const int i = 2 * p - 1, r = p - 1;
        const K2Quad<uint32_t> q = k2_pair_pixels(k2_pair_samples(r, k, PU, PV), yat(i, 2 * k), yat(i, 2 * k + 1), yat(i + 1, 2 * k), yat(i + 1, 2 * k + 1), blend, px);
        d[(size_t)i * w] = q.a0; d[(size_t)i * w + 1] = q.a1; d[(size_t)(i + 1) * w] = q.b0; d[(size_t)(i + 1) * w + 1] = q.b1;
      }
      if ((h - 1) & 1) {
        const int i = h - 1;
        k2_trailing_pixels(i >> 1, k, hw, c.fix != 0, yat(i, 2 * k), yat(0, 2 * k), yat(i, 2 * k + 1), PU, PV, px, d[(size_t)i * w], d[(size_t)i * w + 1]);
      }
    }
    if (fwrite(dst.data(), 4, dst.size(), out) != dst.size()) { fprintf(stderr, "short write\n"); return 2; }
    free(Y); free(U); free(V);
  }
  fclose(in);
  return fclose(out) ? 2 : 0;
}
