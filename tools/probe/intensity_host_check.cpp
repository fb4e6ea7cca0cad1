// Host-side check of csrc/vu_intensity.hip under a sanitizer: vu_intensity_rank over its whole range against 128-bit arithmetic and
// every refusal of the launch entries with fake, never-dereferenced pointers (all of it returns before any GPU call).  Build and run,
// from the repository root, without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -x hip tools/probe/intensity_host_check.cpp vit-unet_amd/csrc/vu_intensity.hip vit-unet_amd/csrc/vu_err.cpp -o intensity_host_check
#include <cstdint>
#include <cstdio>

#include "../../include/vit_unet_amd.h"

static int fails = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } \
  } while (0)

static void rank(unsigned long long N, unsigned pn, unsigned pd) {
  unsigned long long k = 0;
  unsigned r = 0;
  EXPECT(vu_intensity_rank(N, pn, pd, &k, &r) == 0);
  const unsigned __int128 p = (unsigned __int128)(N - 1) * pn;
  EXPECT(k == (unsigned long long)(p / pd) && r == (unsigned)(p % pd) && r < pd && k <= N - 1);
}

int main() {
  const unsigned long long Ns[] = {1, 2, 3, 1000, 16777216, 4294967294ull, 4294967295ull};
  const unsigned pds[] = {1, 2, 3, 7, 100, 999983, 1000000};
  for (unsigned long long N : Ns)
    for (unsigned pd : pds) {
      const unsigned pns[] = {0, 1, pd / 2, pd - 1, pd};
      for (unsigned pn : pns)
        if (pn <= pd) rank(N, pn, pd);
    }
  unsigned long long k = 7;
  unsigned r = 9;
  EXPECT(vu_intensity_rank(0, 1, 2, &k, &r) == -1 && vu_intensity_rank(4294967296ull, 1, 2, &k, &r) == -1);
  EXPECT(vu_intensity_rank(~0ull, 1, 2, &k, &r) == -1);
  EXPECT(vu_intensity_rank(5, 1, 0, &k, &r) == -1 && vu_intensity_rank(5, 3, 2, &k, &r) == -1);
  EXPECT(vu_intensity_rank(5, 1, 1000001, &k, &r) == -1 && vu_intensity_rank(5, 4294967295u, 4294967295u, &k, &r) == -1);
  EXPECT(vu_intensity_rank(5, 1, 2, nullptr, &r) == -1 && vu_intensity_rank(5, 1, 2, &k, nullptr) == -1);
  EXPECT(k == 7 && r == 9);
  int a = 0, b = 0, c = 0;
  EXPECT(vu_intensity_geometry(&a, &b, &c) == 0 && a >= -32768 && b >= 0 && a + b <= 32768 && c > 0);
  EXPECT(vu_intensity_geometry(nullptr, &b, &c) == -1 && vu_intensity_geometry(&a, nullptr, &c) == -1 && vu_intensity_geometry(&a, &b, nullptr) == -1);
  const uintptr_t P = (uintptr_t)1 << 24;
  auto p = [&](int i, int off = 0) { return (void*)(P * i + off); };
  auto hist = [&](void* vol, void* mask, void* h, void* box, int D, int H, int W, int select, int label) {
    return vu_intensity_hist((const int16_t*)vol, (const uint8_t*)mask, (uint32_t*)h, (int32_t*)box, D, H, W, select, 0, label, nullptr);
  };
  EXPECT(hist(nullptr, p(2), p(3), p(4), 2, 8, 12, 0, -1) == -1);
  EXPECT(hist(p(1), p(2), nullptr, p(4), 2, 8, 12, 0, -1) == -1);
  EXPECT(hist(p(1), p(2), p(3), p(4), 2, 8, 12, -1, -1) == -1 && hist(p(1), p(2), p(3), p(4), 2, 8, 12, 3, -1) == -1);
  EXPECT(hist(p(1), nullptr, p(3), p(4), 2, 8, 12, 2, -1) == -1);
  EXPECT(hist(p(1), p(2), p(3), p(4), 2, 8, 12, 2, 256) == -1);
  EXPECT(hist(p(1), p(2), p(3), p(4), 0, 8, 12, 0, -1) == -1 && hist(p(1), p(2), p(3), p(4), 2, -8, 12, 0, -1) == -1);
  EXPECT(hist(p(1), p(2), p(3), p(4), 2, 8, 0, 0, -1) == -1);
  EXPECT(hist(p(1), p(2), p(3), p(4), 1024, 2048, 2048, 0, -1) == -1);                         // exactly 2^32
  EXPECT(hist(p(1), p(2), p(3), p(4), 65536, 65536, 1, 0, -1) == -1);
  EXPECT(hist(p(1), p(2), p(3), p(4), 2147483647, 2147483647, 2147483647, 0, -1) == -1);      // the 64-bit intermediates
  EXPECT(hist(p(1), p(2), p(3, 2), p(4), 2, 8, 12, 0, -1) == -1 && hist(p(1), p(2), p(3), p(4, 1), 2, 8, 12, 0, -1) == -1);
  unsigned pn[4] = {0, 5000, 500000, 1000000}, pd[4] = {1000000, 1000000, 1000000, 1000000};
  auto stats = [&](void* h, unsigned* n, unsigned* d, int nq, void* s) {
    return vu_intensity_stats((const uint32_t*)h, n, d, nq, (long long*)s, nullptr);
  };
  EXPECT(stats(nullptr, pn, pd, 4, p(5)) == -1 && stats(p(3), pn, pd, 4, nullptr) == -1);
  EXPECT(stats(p(3), pn, pd, -1, p(5)) == -1 && stats(p(3), pn, pd, 5, p(5)) == -1);
  EXPECT(stats(p(3), nullptr, pd, 1, p(5)) == -1 && stats(p(3), pn, nullptr, 1, p(5)) == -1);
  EXPECT(stats(p(3, 2), pn, pd, 4, p(5)) == -1 && stats(p(3), pn, pd, 4, p(5, 4)) == -1);
  for (int j = 0; j < 4; ++j) {       // a bad quantile at every position; nq stops the reading before it
    unsigned d2[4] = {1000000, 1000000, 1000000, 1000000}, n2[4] = {0, 5000, 500000, 1000000};
    d2[j] = 0;
    EXPECT(stats(p(3), n2, d2, 4, p(5)) == -1);
    d2[j] = 1000001;
    EXPECT(stats(p(3), n2, d2, 4, p(5)) == -1);
    d2[j] = 1000000; n2[j] = 1000001;
    EXPECT(stats(p(3), n2, d2, 4, p(5)) == -1);
  }
  std::printf(fails ? "intensity_host_check: %d FAILED\n" : "intensity_host_check: ok\n", fails);
  return fails ? 1 : 0;
}
