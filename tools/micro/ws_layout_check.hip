// Host-only check of the workspace layouts of csrc/hip/block_layout.hpp (solve_layout,
// evd_alone_layout, quad_chain_layout) under AddressSanitizer + UBSan: every
// area of a layout is filled with its own byte inside a heap buffer of exactly
// the reported size, then read back.  An area that overlaps another reads back
// wrong; one that runs past the reported size is an ASan heap overflow.  The
// area sizes are stated here independently of the layout routines.  No kernel
// is launched and no GPU is needed; the program holds the layout header alone
// (no kernel, no C entry point, nothing of the library to link).
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined
//     -Xarch_host -fno-sanitize-recover=undefined -I svd-jacobi-mpi-cuda_amd/csrc/include
//     -I svd-jacobi-mpi-cuda_amd/csrc/hip tools/micro/ws_layout_check.hip
//     -o tools/micro/ws_layout_check -fsanitize=address,undefined
#include "block_layout.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

struct Area {
  const char* name;
  void* p;
  size_t bytes;
};

static int check(const char* what, const std::vector<Area>& areas, char* base, size_t size) {
  for (size_t i = 0; i < areas.size(); ++i) {
    const Area& a = areas[i];
    if (!a.p || ((char*)a.p - base) % 256 || (i && a.p <= areas[i - 1].p)) {
      printf("%s: area %s is null, misaligned or out of order\n", what, a.name);
      return 1;
    }
    memset(a.p, (int)i + 1, a.bytes);
  }
  for (size_t i = 0; i < areas.size(); ++i) {
    const unsigned char* q = (const unsigned char*)areas[i].p;
    if (areas[i].bytes && (q[0] != i + 1 || q[areas[i].bytes - 1] != i + 1)) {
      printf("%s: area %s overlaps a neighbour\n", what, areas[i].name);
      return 1;
    }
  }
  const Area& last = areas.back();
  if ((char*)last.p + last.bytes > base + size) return 1;  // (ASan has already said so)
  return 0;
}

template <typename T>
static int solve_case(int W, int P, int m_pad, bool quad, int mma) {
  const size_t size = svdj::solve_ws_bytes<T>(W, P, m_pad, quad);
  std::vector<char> buf(size);
  svdj::Chain<T> c{};
  c.P = P;
  c.g = svdj::make_geometry(W, P, m_pad, 0, mma);
  const size_t used = svdj::solve_layout(c, buf.data(), W, quad);
  if (used > size) return 1;
  const size_t e = sizeof(T), p = P, ww = (size_t)W * W;
  std::vector<Area> a = {{"slabs", c.slabs, p * c.g.gchunks * 4 * ww * e},
                         {"Qb0", c.Qb[0], p * 4 * ww * e}, {"Qb1", c.Qb[1], p * 4 * ww * e},
                         {"skipb0", c.skipb[0], p * 4}, {"skipb1", c.skipb[1], p * 4},
                         {"rec", c.rec, p * svdj::kCrossMaxInner * ww * e}, {"nsteps", c.nsteps, p * 4}};
  if (quad && svdj::has_quad(e, W)) {
    const size_t t = (size_t)(P / 2 > 0 ? P / 2 : 1) * 256 * 256 * 3 * 2;  // 3 bf16 parts
    a.insert(a.end(), {{"qslabs", c.qslabs, 3 * p * c.g.qgch * ww * 4}, {"qred", c.qred, 3 * p * ww * 4},
                       {"T1", c.T1, p * 4 * ww * 8}, {"upd", c.upd, p * ww * 4},
                       {"Ts0", c.Ts[0], t}, {"Ts1", c.Ts[1], t},
                       {"skip10", c.skip1[0], p * 4}, {"skip11", c.skip1[1], p * 4},
                       {"skip20", c.skip2[0], p * 4}, {"skip21", c.skip2[1], p * 4}});
  } else if (c.qslabs || c.Ts[0]) {
    return 1;
  }
  // the chunk sums of the cross slabs lie behind them, inside the slab area
  if (c.xsum != c.slabs + p * c.g.gchunks * ww || (c.xsum + p * ww) > c.slabs + p * c.g.gchunks * 4 * ww)
    return 1;
  return check("solve", a, buf.data(), size);
}

template <typename T>
static int evd_case(int W, int P, int nchunk) {
  const size_t size = svdj::evd_alone_ws_bytes<T>(W, P, nchunk);
  std::vector<char> buf(size);
  svdj::Chain<T> c{};
  c.P = P;
  c.g.gchunks = nchunk;
  if (svdj::evd_alone_layout(c, buf.data(), W) != size) return 1;
  const size_t e = sizeof(T), p = P, ww = (size_t)W * W;
  return check("evd_alone", {{"slabs", c.slabs, p * nchunk * 4 * ww * e},
                             {"rec", c.rec, p * svdj::kCrossMaxInner * ww * e},
                             {"nsteps", c.nsteps, p * 4}}, buf.data(), size);
}

int main() {
  int bad = 0, n = 0;
  for (int W : {32, 64})
    for (int P : {1, 2, 8, 16, 31, 32, 64, 128})
      for (int m_pad : {128, 256, 4096, 16384})
        for (int quad = 0; quad < 2; ++quad)
          for (int mma = 0; mma < 2; ++mma, n += 2)
            bad += solve_case<float>(W, P, m_pad, quad, mma) + solve_case<double>(W, P, m_pad, quad, 0);
  for (int W : {32, 64})
    for (int P : {1, 2, 8, 64})
      for (int nchunk : {1, 4, 9, 32}) {
        bad += evd_case<float>(W, P, nchunk) + evd_case<double>(W, P, nchunk);
        n += 2;
      }
  for (int P : {2, 8, 64}) {
    svdj::Chain<float> c{};
    c.P = P;
    const size_t size = svdj::quad_chain_layout(c, nullptr);  // svdj_quad_chain_workspace_bytes
    std::vector<char> buf(size);
    bad += svdj::quad_chain_layout(c, buf.data()) != size;
    bad += check("quad_chain", {{"qred", c.qred, (size_t)3 * P * 64 * 64 * 4},
                                {"rec", c.rec, (size_t)P * svdj::kCrossMaxInner * 64 * 64 * 4},
                                {"nsteps", c.nsteps, (size_t)P * 4}}, buf.data(), size);
    ++n;
  }
  printf("%d layouts checked, %d bad\n", n, bad);
  return bad != 0;
}
