// The Normalize + /255 step of the denoising input pipeline, shared by csrc/vu_data.hip (vu_denoise_prepare),
// csrc/vu_tile.hip (vu_tile_gather_u8) and csrc/vu_patch.hip (vu_patch_pairs_u8): one definition, so that a window or a
// training patch cut from a large image carries bit for bit the values the validation transform gives the same pixels.
#pragma once
#include "vu_common.h"

// albumentations Normalize(mean, std, max_pixel_value = 255) in float32: (v - mean*255) * (1/(std*255)), then the
// dataset's /255 (dataset.py:66)
static inline float vu_normalize_m255(float mean) { return mean * 255.0f; }
static inline float vu_normalize_rden(float std) { return 1.0f / (std * 255.0f); }
__device__ __forceinline__ float vu_normalize_u8(int v, float m255, float rden) {
  return __fdiv_rn(__fmul_rn(__fsub_rn((float)v, m255), rden), 255.f);
}
// the clean image is divided as uint8/255. (float64) and cast to float32 by unpack (dataset.py:66,80)
__device__ __forceinline__ float vu_unit_u8(int v) { return (float)__ddiv_rn((double)v, 255.0); }

// the intensity window of the segmentation input pipeline (vu_seg_prepare, and vu_tile_gather_i16 of csrc/vu_segtile.hip):
// x = clip((v - lo) / range, 0, 1) with range = hi - lo in float32, every operation rounded once
__device__ __forceinline__ float vu_window_i16(int v, float lo, float range) {
  return fminf(fmaxf(__fdiv_rn(__fsub_rn((float)v, lo), range), 0.f), 1.f);
}
