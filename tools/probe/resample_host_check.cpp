// Host-side check of csrc/vu_resample.hip under a sanitizer: the table entries over a grid of lengths and every refusal of the
// launch entries with fake, never-dereferenced pointers (all of it returns before any GPU call).  Build and run, from the repository
// root, without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -x hip tools/probe/resample_host_check.cpp vit-unet_amd/csrc/vu_resample.hip vit-unet_amd/csrc/vu_err.cpp -o resample_host_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/vit_unet_amd.h"

static int fails = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } \
  } while (0)

static void tables(int n_in, int n_out) {
  const int Q = 1 << 15;
  std::vector<int> i0(n_out), w(n_out), src(n_out);   // exactly n_out entries: a write past the end is the sanitizer's to find
  EXPECT(vu_resample_axis_linear(n_in, n_out, i0.data(), w.data(), n_out) == n_out);
  EXPECT(vu_resample_axis_nearest(n_in, n_out, src.data(), n_out) == n_out);
  for (int i = 0; i < n_out; ++i) {
    EXPECT(i0[i] >= 0 && i0[i] <= n_in - 1 && w[i] >= 0 && w[i] <= Q && src[i] >= 0 && src[i] <= n_in - 1);
    if (n_in == n_out) EXPECT(i0[i] == i && w[i] == 0 && src[i] == i);
  }
  EXPECT(vu_resample_axis_linear(n_in, n_out, i0.data(), w.data(), n_out - 1) == -1);
  EXPECT(vu_resample_axis_nearest(n_in, n_out, src.data(), n_out - 1) == -1);
}

int main() {
  for (int a = 1; a <= 40; ++a)
    for (int b = 1; b <= 40; ++b) tables(a, b);
  tables(512, 307); tables(307, 512); tables(3, 1000);
  tables(2147483647, 7); tables(7, 100000); tables(1, 1);
  {   // the largest lengths: the 64-bit intermediates of the last entries
    const int n = 2147483647;
    std::vector<int> i0(1), w(1);
    EXPECT(vu_resample_axis_linear(n, n, i0.data(), w.data(), 1) == -1);
  }
  int tx = 0, ty = 0, tz = 0;
  EXPECT(vu_resample_geometry(&tx, &ty, &tz) == 0 && tx > 0 && ty > 0 && tz > 0);
  EXPECT(vu_resample_geometry(nullptr, &ty, &tz) == -1);
  const uintptr_t P = (uintptr_t)1 << 24;
  auto p = [&](int k) { return (void*)(P * k); };
  EXPECT(vu_resample_i16(nullptr, (int16_t*)p(2), 2, 8, 12, 3, 5, 9, nullptr) == -1);
  EXPECT(vu_resample_i16((const int16_t*)p(1), nullptr, 2, 8, 12, 3, 5, 9, nullptr) == -1);
  EXPECT(vu_resample_i16((const int16_t*)p(1), (int16_t*)p(2), 0, 8, 12, 3, 5, 9, nullptr) == -1);
  EXPECT(vu_resample_i16((const int16_t*)p(1), (int16_t*)p(2), 2, 8, 12, 3, -5, 9, nullptr) == -1);
  EXPECT(vu_resample_i16((const int16_t*)p(1), (int16_t*)p(2), 2048, 1024, 1024, 3, 5, 9, nullptr) == -1);
  EXPECT(vu_resample_i16((const int16_t*)p(1), (int16_t*)p(2), 2, 8, 12, 2147483647, 2147483647, 2147483647, nullptr) == -1);
  EXPECT(vu_resample_i16((const int16_t*)p(1), (int16_t*)p(1), 2, 8, 12, 3, 5, 9, nullptr) == -1);
  EXPECT(vu_resample_u8_nearest((const uint8_t*)p(1), (uint8_t*)p(1), 2, 8, 12, 3, 5, 9, nullptr) == -1);
  EXPECT(vu_resample_u8_nearest((const uint8_t*)p(1), (uint8_t*)p(2), 2, 8, 0, 3, 5, 9, nullptr) == -1);
  EXPECT(vu_resample_f32_scratch_bytes(3, 5, 9) == 36 && vu_resample_f32_scratch_bytes(0, 5, 9) == 0);
  EXPECT(vu_resample_f32_scratch_bytes(2147483647, 2147483647, 2147483647) > 0);
  auto f32 = [&](void* in, void* truth, void* out, void* mask, void* counts, void* scratch, size_t nb, float zthr, int label) {
    return vu_resample_f32((const float*)in, (const uint8_t*)truth, (float*)out, (uint8_t*)mask, (unsigned long long*)counts, scratch, nb,
                           2, 8, 12, 3, 5, 9, zthr, label, nullptr);
  };
  EXPECT(f32(nullptr, p(2), p(3), p(4), p(5), p(6), 36, 0.f, -1) == -1);
  EXPECT(f32(p(1), p(2), nullptr, nullptr, nullptr, p(6), 36, 0.f, -1) == -1);
  EXPECT(f32(p(1), nullptr, p(3), p(4), p(5), p(6), 36, 0.f, -1) == -1);
  EXPECT(f32(p(1), p(2), p(3), p(4), p(5), p(6), 35, 0.f, -1) == -1);
  EXPECT(f32(p(1), p(2), p(3), p(4), p(5), nullptr, 36, 0.f, -1) == -1);
  EXPECT(f32(p(1), p(2), p(3), p(4), p(5), p(6), 36, 0.f, 256) == -1);
  EXPECT(f32(p(1), p(2), p(3), p(4), p(5), p(6), 36, __builtin_nanf(""), -1) == -1);
  EXPECT(f32(p(1), p(2), p(1), p(4), p(5), p(6), 36, 0.f, -1) == -1);
  EXPECT(f32(p(1), p(2), p(3), p(3), p(5), p(6), 36, 0.f, -1) == -1);
  EXPECT(f32(p(1), p(2), p(3), p(4), p(5), p(5), 36, 0.f, -1) == -1);
  std::printf(fails ? "resample_host_check: %d FAILED\n" : "resample_host_check: ok\n", fails);
  return fails ? 1 : 0;
}
