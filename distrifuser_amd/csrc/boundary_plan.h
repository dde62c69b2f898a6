// Host-side launch arithmetic of the NCHW <-> token transposing kernels
// (gn_apply_tokens, tokens_add_nchw in groupnorm.hip). Plain C++, no HIP
// types, so it also compiles for the CPU on its own.
#pragma once

#include <cstdint>

// Vector path: 64 channels x 64 pixels of a 16-bit type per 256-thread block,
// 16-byte global accesses on both sides. Scalar path: 32 x 32 elements of any
// type, any C and HW.
constexpr int BOUNDARY_VEC_TILE = 64;
constexpr int BOUNDARY_SCALAR_TILE = 32;
constexpr int BOUNDARY_THREADS = 256;
constexpr int64_t BOUNDARY_MAX_GRID_YZ = 65535;

struct BoundaryPlan {
    bool ok;     // false: nothing to launch (empty tensor) or grid out of range
    bool empty;  // N * C * HW == 0
    bool vec;
    int tile;  // channels and pixels per block
    int64_t grid_x, grid_y, grid_z;  // pixel tiles, channel tiles, samples
};

// elem_size: bytes per element. aligned16: every base pointer is 16-byte
// aligned and every stride that is not the innermost one is a multiple of
// 16 bytes (the caller looks at its own tensors).
inline BoundaryPlan boundary_plan(int64_t n, int64_t c, int64_t hw, int elem_size,
                                  bool aligned16) {
    BoundaryPlan p{};
    if (n < 0 || c < 0 || hw < 0) return p;
    p.empty = n == 0 || c == 0 || hw == 0;
    p.vec = elem_size == 2 && aligned16 && hw % 8 == 0 && c % 8 == 0;
    p.tile = p.vec ? BOUNDARY_VEC_TILE : BOUNDARY_SCALAR_TILE;
    p.grid_x = (hw + p.tile - 1) / p.tile;
    p.grid_y = (c + p.tile - 1) / p.tile;
    p.grid_z = n;
    p.ok = !p.empty && p.grid_x <= INT32_MAX && p.grid_y <= BOUNDARY_MAX_GRID_YZ &&
           p.grid_z <= BOUNDARY_MAX_GRID_YZ;
    return p;
}

// A [N, C, H, W] tensor whose (H, W) plane is contiguous: the batch and
// channel strides are free. Strides in elements.
inline bool boundary_plane_contiguous(const int64_t sizes[4], const int64_t strides[4]) {
    const bool w_ok = sizes[3] <= 1 || strides[3] == 1;
    const bool h_ok = sizes[2] <= 1 || strides[2] == sizes[3];
    return w_ok && h_ok;
}
