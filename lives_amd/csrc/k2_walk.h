// k2_walk.h -- K2's chroma walk, written once: which chroma sample feeds which pixel in convert_yuv420p_to_rgb_frame (src/colourspace.c:3260-3904).
// The kernels that convert planar 4:2:0 / 4:2:2 to RGB call it: yuv.hip (the 4:2:2 fast cell of k_yuv420p_to_rgb_s), flat.hip (flat_cell's row 0, flat_row422)
// and pixbuf.hip (every row of k_pb_half<.., YUV>).  tests/test_k2_walk_cpu.py holds this header alone against the oracle's K2 on the CPU.
// Plain C++17: no HIP header is needed, and the arithmetic is the caller's -- blend(s1, s2, top, bot), the blends of two doubled sums for the first and the second
// row of a pair ((2 s1 + s2) / 3 and (s1 + 2 s2) / 3 on halves, or s1 >> 1 and s2 >> 1 with pb_quality LOW, with whatever clamp the caller's tables need), and a
// px(luma, iu, iv) whose result type is the caller's own.  The luma is whatever px takes: a value, or the byte's address.
//
// A frame is walked in units: unit 0 = row 0; unit p >= 1 = rows (2p - 1, 2p) while 2p <= H - 1; then (even H) the trailing row H - 1.  A cell is one chroma
// column k of a unit: two pixels (2k, 2k + 1) of one row or a 2 x 2 quad.  pu(row, col) / pv(row, col) read a chroma sample.
//
// The reference's rules, kept bit for bit:
//   row 0 (:3399-3443)
//     a  the left pixel averages column k with k - 1, the right one with k + 1, both clamped into the row (kp, kn)
//   rows (2p - 1, 2p), chroma rows r = p - 1 and r + 1 (:3445-3554)
//     b  left pixel, U: the second row's sum is rebuilt from the first row, so both rows blend (su, su) with su = U(r, k) + U(r, k - 1)  (:3461)
//     c  left pixel, V: V(r, k) pairs with the PREVIOUS V of row r + 1, V(r + 1, k - 1), and V(r + 1, k) with a "last V" frozen at column 0, V(r + 1, 0)  (:3544)
//     d  at column 0 the left sample is the centre sample of row r: U(r, -1) := U(r, 0), V(r + 1, -1) := V(r, 0)  (:3447-3452)
//     e  the right pixel reads column k + 1 as it is: the row's last cell reads one sample past the row's end (the next row's first sample), and the plane's
//        last row one byte past the plane -- clamped to the plane's last byte BY THE ACCESSOR (or by the caller's window load)
//     f  the top row takes the blend of (s1, s2) and the bottom row that of (s2, s1), s1 the sum from chroma row r and s2 the one from row r + 1
//   the trailing row H - 1 of an even height, r = (H - 1) >> 1 (:3556-3592)
//     g  LGPU_YUV_FIX_EDGES: as row 0 on chroma row r
//     h  otherwise the reference's one-thread walk: the left pixel's LUMA comes from row 0 and its this / last samples from chroma row 0, except that
//        {row r, column 0} stands in for column 0 (this) and for every column below 2 (last); the right pixel is row r's, its next sample clamped into the row
//   a 4:2:2 row i (:3593-3640 / :3858-3901)
//     i  this and last are seeded from chroma row i >> 1: {row i >> 1, column 0} stands in for column 0 (this, of BOTH pixels) and for every column below 2
//        (last); the next sample is column k + 1 as it is (rule e)
// Kernels that load a cell's samples as a window (the 4:2:2 fast cell of k_yuv420p_to_rgb_s, the interior path of flat_row422, k_pb_half) unpack the window into
// the same named samples and call the same k2_pair_pixels / k2_row_pixels; where they patch the window for rule a, d, h or i they name the rule.
// Where going through a function of this header cost a kernel registers, code size or time against its earlier machine code, the site keeps its own text and a
// comment naming the function and rules it repeats (yuv.hip: yuv420_cell, yuv422_cell, the prefetched cell of k_yuv420p_to_rgb, the 4:2:0 fast cell of
// k_yuv420p_to_rgb_s; flat.hip: flat_cell's row pair and trailing row, flat_row422's seeded path; profiles/r18/k2_walk.md has the figures): change those with the rule.
#ifndef LGPU_K2_WALK_H
#define LGPU_K2_WALK_H

#if defined(__HIPCC__)
#define K2_FN __host__ __device__ __forceinline__
#else
#define K2_FN inline
#endif

namespace lgpu {

// ---- a row pair -----------------------------------------------------------------------------------------------------------------------------
// the samples of cell k: l / c / n = column k - 1 / k / k + 1; no digit = chroma row r, 1 = chroma row r + 1; v1_0 = V(r + 1, 0)
template <class S> struct K2Pair { S u_l, u_c, u_n, u1_c, u1_n, v_c, v_n, v1_l, v1_c, v1_n, v1_0; };
template <class R> struct K2Quad { R a0, a1, b0, b1; };      // top row's left and right pixel, bottom row's

template <class PU, class PV>
K2_FN auto k2_pair_samples(int r, int k, PU &&pu, PV &&pv) -> K2Pair<decltype(pu(r, k))> {
  K2Pair<decltype(pu(r, k))> s;
  s.u_c = pu(r, k); s.v_c = pv(r, k); s.v1_c = pv(r + 1, k);
  s.u_l = k ? pu(r, k - 1) : s.u_c;                          // rule d
  s.v1_l = k ? pv(r + 1, k - 1) : s.v_c;                     // rule d
  s.v1_0 = pv(r + 1, 0);                                     // rule c
  s.u_n = pu(r, k + 1); s.u1_c = pu(r + 1, k); s.u1_n = pu(r + 1, k + 1);      // rule e
  s.v_n = pv(r, k + 1); s.v1_n = pv(r + 1, k + 1);
  return s;
}

// y00 y01 / y10 y11: the quad's luma
template <class S, class Y, class Blend, class Px>
K2_FN auto k2_pair_pixels(const K2Pair<S> &s, Y y00, Y y01, Y y10, Y y11, Blend &&blend, Px &&px) -> K2Quad<decltype(px(y00, s.u_c, s.u_c))> {
  K2Quad<decltype(px(y00, s.u_c, s.u_c))> q;
  S ut, ub, vt, vb;
  // left pixel (rules b, c)
  blend(s.u_c + s.u_l, s.u_c + s.u_l, ut, ub);
  blend(s.v_c + s.v1_l, s.v1_c + s.v1_0, vt, vb);
  q.a0 = px(y00, ut, vt); q.b0 = px(y10, ub, vb);
  // right pixel
  blend(s.u_c + s.u_n, s.u1_c + s.u1_n, ut, ub);
  blend(s.v_c + s.v_n, s.v1_c + s.v1_n, vt, vb);
  q.a1 = px(y01, ut, vt); q.b1 = px(y11, ub, vb);
  return q;
}

// ---- a single row of pixel pairs: row 0, the trailing row, a 4:2:2 row -------------------------------------------------------------------------
// this / last / next: columns k, k - 1, k + 1 as the rules below pick them
template <class S> struct K2Row { S tu, tv, lu, lv, nu, nv; };

// rules a and g: cell k of chroma row `row`, hw cells wide
template <class PU, class PV>
K2_FN auto k2_row_edge(int row, int k, int hw, PU &&pu, PV &&pv) -> K2Row<decltype(pu(row, k))> {
  const int kp = k ? k - 1 : 0, kn = (k + 1 < hw) ? k + 1 : hw - 1;
  K2Row<decltype(pu(row, k))> s;
  s.tu = pu(row, k); s.tv = pv(row, k);
  s.lu = pu(row, kp); s.lv = pv(row, kp);
  s.nu = pu(row, kn); s.nv = pv(row, kn);
  return s;
}
// the seeded this / last of rules h and i: chroma row `row`, with {seed, 0} in place of column 0 (this) and of the columns below 2 (last)
template <class S, class PU, class PV>
K2_FN void k2_row_seeded(K2Row<S> &s, int row, int seed, int k, PU &&pu, PV &&pv) {
  s.tu = k ? pu(row, k) : pu(seed, 0); s.tv = k ? pv(row, k) : pv(seed, 0);
  s.lu = (k >= 2) ? pu(row, k - 1) : pu(seed, 0); s.lv = (k >= 2) ? pv(row, k - 1) : pv(seed, 0);
}
// rule i: row i of a 4:2:2 frame
template <class PU, class PV>
K2_FN auto k2_row_422(int i, int k, PU &&pu, PV &&pv) -> K2Row<decltype(pu(i, k))> {
  K2Row<decltype(pu(i, k))> s;
  k2_row_seeded(s, i, i >> 1, k, pu, pv);
  s.nu = pu(i, k + 1); s.nv = pv(i, k + 1);                  // rule e
  return s;
}

// the two pixels of a row: px(y0, (this + last) >> 1, ..) and px(y1, (this + next) >> 1, ..)
template <class S, class Y, class Px>
K2_FN auto k2_row_left(const K2Row<S> &s, Y y0, Px &&px) -> decltype(px(y0, s.tu, s.tv)) { return px(y0, (s.tu + s.lu) >> 1, (s.tv + s.lv) >> 1); }
template <class S, class Y, class Px>
K2_FN auto k2_row_right(const K2Row<S> &s, Y y1, Px &&px) -> decltype(px(y1, s.tu, s.tv)) { return px(y1, (s.tu + s.nu) >> 1, (s.tv + s.nv) >> 1); }
template <class S, class Y, class Px, class R>
K2_FN void k2_row_pixels(const K2Row<S> &s, Y y0, Y y1, Px &&px, R &p0, R &p1) {
  p0 = k2_row_left(s, y0, px);
  p1 = k2_row_right(s, y1, px);
}

// rules g and h: the trailing row, chroma row r.  y0 / y1: the two pixels' luma in the row itself, y0_row0: the left pixel's luma in row 0.
// The right pixel is always the row's own (e); without fix_edges the left one takes the seeded walk over chroma row 0 instead
template <class Y, class PU, class PV, class Px, class R>
K2_FN void k2_trailing_pixels(int r, int k, int hw, bool fix_edges, Y y0, Y y0_row0, Y y1, PU &&pu, PV &&pv, Px &&px, R &p0, R &p1) {
  const K2Row<decltype(pu(r, k))> e = k2_row_edge(r, k, hw, pu, pv);
  if (fix_edges) p0 = k2_row_left(e, y0, px);
  else {
    K2Row<decltype(pu(r, k))> s;
    k2_row_seeded(s, 0, r, k, pu, pv);
    p0 = k2_row_left(s, y0_row0, px);
  }
  p1 = k2_row_right(e, y1, px);
}

}  // namespace lgpu
#endif
