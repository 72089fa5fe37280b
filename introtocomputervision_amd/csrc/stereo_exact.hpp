// stereo_exact.hpp -- the exact-sum stereo path for 8-bit-valued images (stereo_exact.hip), as stereo.hip sees it.
#pragma once
#include "common.hpp"
#include "stereo_float.hpp"

namespace micv {

struct StereoExactArgs {
    const float *left, *right;  // the caller's f32 images (read by the pack pre-pass only)
    int stride, rows, cols, min_d, max_d, wcols;
    // the u8 entries: byte images of `batch` pairs (read by the u8 pack pre-pass only), pair i at base + i * pair stride,
    // row pitches in bytes, no alignment anywhere; null for an f32 call
    const uint8_t *left8, *right8;
    size_t lstride8, rstride8, lpair8, rpair8;
    // A launch covers `batch` pairs of one size: strip s of the launch (lplan, rpack) is strip s % spp of pair s / spp,
    // row y of pair i is row i * rows + y of A and B, its disparity map starts at disp + i * dpair.  (1, all strips, 0 for a
    // single pair: everything below then reads as it did before there was a batch.)
    int batch, spp;
    size_t dpair;
    uint32_t *lplan;  // [strip][column + R][8]: packed rows of `left`, one 32-byte record per column (scalar loads)
    int lcols;        // records per strip: columns -R .. lcols - R - 1, clamped copies outside the image
    int qlo, qhi;     // columns the pre-pass visits
    uint32_t *rpack;  // [strip][word][colsP]: packed rows of `right`
    int colsP;
    int32_t *A;  // [rows][cols]  window energy of left at output x (MIN_SSD_5E6 only, else null)
    int32_t *B;  // [rows][nB]    window energy of right at position p = x + d, p - min_d in [0, nB)
    int nB;
    unsigned *flag;  // holds `epoch` once a pixel of this call was found not to be an integer in 0..255
    unsigned epoch;
    int8_t *disp;
    int dstride;
    int X, nxs, ntiles;  // output columns per wave, strips per row of strips, waves
    int min_ssd_5e6;
    int nblk_exact, fgx;  // workgroups of exact-sum tiles in the launch; the float tiles behind them: fgx strips of columns per row of tiles
};

// Whether the exact path has a kernel for this call at all (radius, flags); the images decide on the device.
bool stereo_exact_covers(int rad, int flags, bool ncc);
// Bytes of planes of a launch of `batch` pairs TILED AS a launch of `tile_batch` pairs is (0 = batch).  The layout of a pair
// (columns per wave, plan records per strip) follows from the tiling, and the tiling from the number of strips it prices:
// the pieces of a large batch are all tiled as its full piece, so that one reservation holds every one of them.
size_t stereo_exact_scratch(int rows, int cols, int rad, int min_d, int max_d, int wcols, int flags, int wave_slots3,
                            int batch = 1, int tile_batch = 0);
// Enqueues pre-pass + search (wave_slots3: waves the device holds at three per SIMD).  The search launch carries the
// float kernel's tiles for the same call (`f`, 8 or 10 rows per wave) as trailing workgroups: nothing else to launch.  `scratch` holds stereo_exact_scratch() bytes.
int stereo_exact_launch(hipStream_t s, void *scratch, const float *left, const float *right, int rows, int cols,
                        int stride, int rad, int min_d, int max_d, int flags, int wcols, int8_t *disp, int dstride,
                        unsigned *flag, unsigned epoch, int wave_slots3, const StereoArgs &f, bool rows10);

// The same two launches for `batch` pairs of BYTE images (the u8 entry points of stereo.hip): the u8 pre-pass packs all
// pairs in one launch and tests nothing, the search launch holds the exact-sum tiles of all pairs and no float tiles.
// `never` is a word nobody writes and that holds 0 (the search's flag test then never selects the float images).
// `flags` without ROLLING; stereo_exact_covers(rad, flags, false) must hold.  `scratch` holds `scratch_bytes`; a launch
// whose planes (`batch` pairs tiled as `tile_batch`) would not fit is refused before anything is enqueued.
int stereo_exact_launch_u8(hipStream_t s, void *scratch, size_t scratch_bytes, const uint8_t *left, size_t lpair, size_t lstride,
                           const uint8_t *right, size_t rpair, size_t rstride, int batch, int tile_batch, int rows, int cols,
                           int rad, int min_d, int max_d, int flags, int wcols, int8_t *disp, size_t dpair, int dstride,
                           unsigned *never, int wave_slots3);

}  // namespace micv
