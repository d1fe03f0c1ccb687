// The eight orientations of an image (the dihedral group of the square) and the geometric self-ensemble built on them
// (mz_dihedral(), mz_ensemble_add(), mz_ensemble_finish(): include/mewzoom_hip.h).  No reference counterpart in model.py: the flip is
// the reference's RandomHorizontalFlip augmentation (pretrain.py:148); the ensemble is the "+" variant of the super-resolution papers.
//
// THE TRANSFORM, stated here once (the device kernels of mz_dihedral.hip, the host entries of mz_image.cpp and tests/dihedral_main.cpp
// compile this source).  Orientation k = 0..7 has three bits: bit 0 reverses columns, bit 1 reverses rows, bit 2 exchanges rows and
// columns and is applied LAST:
//     T(x, k)[b, c, i, j] = x[b, c, si, sj]    (p, q) = k & 4 ? (j, i) : (i, j)    si = k & 2 ? H - 1 - p : p    sj = k & 1 ? W - 1 - q : q
// for x of H x W pixels; T(x, k) has W x H pixels when k & 4.  inverse(k) = k for k < 4 (flips undo themselves), else
// 4 | (k & 1) << 1 | (k & 2) >> 1 (a transposition exchanges the two flip bits: 5 and 6, the two quarter turns, are each other's
// inverse; 4 and 7, the two diagonal mirrors, their own).  The transform moves elements and never changes them.
//
// This header needs no HIP header: plain g++ compiles it (tests/dihedral_main.cpp runs it under the sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mz_view.h"

#ifdef __HIPCC__
#define MZ_HD __host__ __device__
#else
#define MZ_HD
#endif

namespace mz {

MZ_HD inline bool dihedral_valid(int k) { return k >= 0 && k <= 7; }

// negative outside 0..7
MZ_HD inline int dihedral_inverse(int k) {
    if (!dihedral_valid(k)) return -1;
    return k < 4 ? k : 4 | ((k & 1) << 1) | ((k & 2) >> 1);
}

// the shape of T(x, k) of an H x W image
MZ_HD inline void dihedral_shape(int k, int H, int W, int* Ho, int* Wo) {
    *Ho = (k & 4) ? W : H;
    *Wo = (k & 4) ? H : W;
}

// the element (si, sj) of the H x W image that T(x, k) has at (i, j)
MZ_HD inline void dihedral_source(int k, int H, int W, int i, int j, int* si, int* sj) {
    const int p = (k & 4) ? j : i, q = (k & 4) ? i : j;
    *si = (k & 2) ? H - 1 - p : p;
    *sj = (k & 1) ? W - 1 - q : q;
}

// ---- the kernels' side (mz_dihedral.hip) ------------------------------------------------------------------------------------------
// One tile skeleton moves every orientation: a workgroup of kDihedralThreads threads takes one kDihedralTile x kDihedralTile pixel
// tile of one plane of the DESTINATION, finds the source rectangle that lands on it (two calls of dihedral_source: the tile's corners),
// loads that rectangle into LDS row by row of the SOURCE, and stores the tile row by row of the DESTINATION, each element from the LDS
// slot dihedral_source names.  Loads and stores both run along the unit-stride axis of their view (lanes along columns; along rows for
// a view whose row stride is the unit one, e.g. a transposed tensor); the exchange of the two axes happens in LDS alone.
//
// LDS: [kDihedralTile][kDihedralPitch] dwords, one dword per element whatever its type (a 16- or 8-bit element travels zero-extended;
// in accumulate mode the dword is the element's float32 value).  Bank of a dword (ds_write / ds_read_b32): (r * 65 + c) % 32 =
// (r + c) % 32.  Loading lanes along c or along r, storing lanes along either: the 32 lanes of a group differ in r + c by 0..31 --
// every bank once.  The 16-byte paths give a lane 4 / 8 / 16 consecutive dwords: per ds instruction the lanes of a group then lie 4 / 8
// / 16 banks apart within a row and one bank apart from row to row, which puts two lanes on a bank (2-way; a power-of-two pitch would
// put all 32 on one).  ds_write_b32 hides a 2-way conflict behind its own register transfer; a 2-way ds_read_b32 still moves dwords at
// 16 times the rate HBM delivers elements to the tile.
constexpr int kDihedralTile = 64;
constexpr int kDihedralPitch = kDihedralTile + 1;  // odd: a column of the tile walks all 32 banks
constexpr int kDihedralThreads = 256;
static_assert(kDihedralThreads == kImageThreads, "grid_ok() (mz_view.h) bounds a grid of workgroups of kImageThreads threads");

enum DihedralMode : int { DM_COPY = 0, DM_ACC = 1 };  // raw elements to a view of the same type; float32 values stored to / added into the accumulator

struct DihedralArgs {
    StridedView src, dst;  // dst: DM_COPY a view of elem; DM_ACC the dense float32 accumulator
    int elem;              // Elem 0..3 of src
    int mode;              // DihedralMode
    int B, Hs, Ws;         // the source's shape
    int k;                 // dst = T(src, k)
    int first;             // DM_ACC: store (nonzero) or add
};
struct EnsembleFinishArgs {
    const float* acc;      // dense [B][3][H][W]
    StridedView out;       // the window's view
    int elem, B, H, W;
    int n, clamp;
    int y0, x0, h, w;
};
// hipError_t values (kept as int: this header stays free of HIP types); hipErrorInvalidValue for a grid beyond what grid_ok() (mz_view.h) can launch
int launch_dihedral(const DihedralArgs& a, void* hip_stream);
int launch_ensemble_finish(const EnsembleFinishArgs& a, void* hip_stream);

// bytes of the accumulator of B results of H x W pixels; false where that is no size_t worth allocating (beyond 2^62)
inline bool ensemble_workspace_bytes(int B, int H, int W, size_t* bytes) {
    const __int128 n = (__int128)12 * B * H * W;
    if (n <= 0 || n > ((__int128)1 << 62)) return false;
    *bytes = (size_t)n;
    return true;
}

}  // namespace mz
