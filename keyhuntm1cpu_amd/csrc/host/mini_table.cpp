#include "mini_table.hpp"

#include <algorithm>
#include <atomic>
#include <thread>

#include "secp_host.hpp"

namespace khb {

namespace {

// p[m + i] = p[i] + p[m] for i = 1 .. n (n <= m; i == m is the doubling), one batch inversion for the step.
void table_step(Pt* p, uint32_t m, uint32_t n, std::vector<Fh>& dx, std::vector<Fh>& scratch) {
  const Pt& Q = p[m];
  const uint32_t adds = n < m ? n : m - 1;       // the distinct-point additions
  dx.resize(adds ? adds : 1);
  scratch.resize(adds ? adds : 1);
  for (uint32_t i = 1; i <= adds; ++i) fe_sub(dx[i - 1], Q.x, p[i].x);
  if (adds) fe_batch_inv(dx.data(), adds, scratch.data());
  for (uint32_t i = 1; i <= adds; ++i) {
    Fh dy, s, x, y;
    fe_sub(dy, Q.y, p[i].y);
    fe_mul(s, dy, dx[i - 1]);
    fe_sqr(x, s);
    fe_sub(x, x, p[i].x);
    fe_sub(x, x, Q.x);
    fe_sub(y, p[i].x, x);
    fe_mul(y, y, s);
    fe_sub(y, y, p[i].y);
    p[m + i] = Pt{x, y};
  }
  if (n == m) p[2 * m] = double_direct(Q);
}

}  // namespace

std::vector<uint8_t> mini_table_be(uint32_t w, int threads) {
  if (w != 4 && w != 8 && w != 16) return {};
  const uint32_t nwin = 256 / w, per = (1u << w) - 1;
  std::vector<uint8_t> out((size_t)64 * nwin * per);
  std::atomic<uint32_t> next{0};
  auto work = [&] {
    std::vector<Pt> p(per + 1);                  // p[d] = d * 2^(w j) * G, p[0] unused
    std::vector<Fh> dx, scratch;
    for (;;) {
      const uint32_t j = next.fetch_add(1);
      if (j >= nwin) break;
      p[1] = mul_g(U256(1).shl((int)(w * j)));
      for (uint32_t m = 1; m < per;) {
        const uint32_t n = std::min(m, per - m);
        table_step(p.data(), m, n, dx, scratch);
        m += n;
      }
      uint8_t* o = out.data() + (size_t)64 * j * per;
      for (uint32_t d = 1; d <= per; ++d) pt_to_be(o + 64 * (size_t)(d - 1), p[d]);
    }
  };
  if (threads < 1) threads = 1;
  if ((uint32_t)threads > nwin) threads = (int)nwin;
  std::vector<std::thread> th;
  for (int t = 1; t < threads; ++t) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  return out;
}

}  // namespace khb
