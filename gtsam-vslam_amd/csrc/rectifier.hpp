// Host object behind vslam_rectifier (rectify.hip): the CV_32F maps of one camera in HBM.  The extractor reads the maps and
// sizes when raw frames are rectified on the way into pyramid level 0 (vslam_extractor::set_images_raw).
#pragma once
#include "common.hpp"

struct vslam_rectifier {
    int device = 0, w = 0, h = 0, sw = 0, sh = 0;      // output (map) size, source size
    hipStream_t stream = nullptr;
    float* d_mapX = nullptr; float* d_mapY = nullptr;  // [h][w], complete once vslam_rectifier_create has returned
    const uint8_t** h_ptrs = nullptr; const uint8_t** d_ptrs = nullptr; int ptrCap = 0;      // [src..., dst...]
};
