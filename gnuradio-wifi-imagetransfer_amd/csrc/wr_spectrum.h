// wr_spectrum.h -- launch interface of the band survey (wr_spectrum.hip; internal, not the C ABI): windowed-FFT power rows of
// a stream, the fold of rows and the band powers of rows, NUMERICS.md rule 36.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wifirx.h"

#define WR_SPEC_ENTRIES 4096    // entries of each of rule 36's tables (wr_spectrum_table.h, generated when the library is built)
#define WR_SPEC_LANES 256       // lanes of a workgroup of spectrum_kernel
#define WR_SPEC_TILE 1024       // points of a tile for n_fft <= 1024: 1024 / n_fft rows side by side (n_fft = 4096: one row)

// The bands of a wifirx_spectrum_bands call, a kernel argument by value: nothing is uploaded for a call.
struct wr_spec_bands {
    uint32_t lo[WIFIRX_SPEC_MAX_BANDS];           // first bin of band b
    uint32_t hi[WIFIRX_SPEC_MAX_BANDS];           // one past its last bin
};

extern "C" {
// n_rows > 0 rows of n_fft bins into rows_out from the samples of `fmt` at in (natural alignment): row r folds the segments
// r * avg .. r * avg + avg - 1, segment s starting at sample s * hop.  The caller has checked n_fft in {64, 256, 1024, 4096},
// window and mode, and that ((n_rows * avg - 1) * hop + n_fft) samples lie at in.  Device pointers that do not overlap.
hipError_t wr_launch_spectrum(hipStream_t st, const void* in, int fmt, float scale, uint32_t n_fft, uint32_t hop, uint32_t avg,
                              int window, int mode, float norm, float* rows_out, uint64_t n_rows);
// n_out > 0 rows: out row q = the fold of rows q * group .. q * group + group - 1, per bin, ascending
hipError_t wr_launch_spectrum_fold(hipStream_t st, const float* rows, uint32_t n_fft, uint64_t group, int mode, float* out,
                                   uint64_t n_out);
// out[r * n_bands + b] = the sum of row r's bins b->lo[b] .. b->hi[b] - 1 (lo < hi <= n_fft), one wave per (row, band)
hipError_t wr_launch_spectrum_bands(hipStream_t st, const float* rows, uint64_t n_rows, uint32_t n_fft, uint32_t n_bands,
                                    const wr_spec_bands* b, float* out);
// the three tables of 4096 entries (host memory, static): twiddle as (re, im) pairs
const float* wr_spectrum_host_hann(void);
const float* wr_spectrum_host_blackman_harris(void);
const float* wr_spectrum_host_twiddle(void);
}
