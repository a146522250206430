// wr_frontend.h -- launch interface of wr_frontend.hip (NUMERICS.md rule 32: DC removal and blind IQ correction; rx_impair)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wifirx.h"

extern "C" {
// the most blocks a call of n samples can touch, whatever the state's sample count: the rows of `table` (5 int64 each)
uint64_t   wr_frontend_table_rows(uint64_t n);
// statistics, apply, state: three launches on `st`.  state, in, out, table: device memory (table: wr_frontend_table_rows(n) rows)
hipError_t wr_launch_frontend(hipStream_t st, const wifirx_frontend_cfg* cfg, wifirx_frontend_state* state, const void* in,
                              int fmt, float scale, uint64_t n, float2* out, int64_t* table, uint32_t n_cu);
hipError_t wr_launch_rx_impair(hipStream_t st, const float2* in, float2* out, uint64_t n, float2 mu, float2 nu, float2 dc,
                               uint32_t n_cu);
}
