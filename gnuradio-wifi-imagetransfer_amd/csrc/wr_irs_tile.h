// wr_irs_tile.h -- the 16-row A tile of the two float32 GEMMs that contract over a row's element products: wr_irs_sweep.hip's
// irs_sweep_kernel and wr_irs_estimate.hip's irs_observe_kernel.  A row is (set r, rho = m L + l); the tile holds the products
// e_n = a_{m,n} b_n of one chunk of 64 elements for 16 rows, as the 128 floats (e_n.re, e_n.im) of the chain.  For a workgroup
// of four waves.
#pragma once
#include "wr_irs_elem.h"

namespace wr {

#define IRS_TILE_CHUNK 64                        // elements per chunk: 128 floats of the chain, 32 steps of 4
#define IRS_TILE_RS    (2 * IRS_TILE_CHUNK + 4)  // LDS row stride in floats: lane (row, kk)'s word at bank 4 row + kk, so the
                                                 // A-operand reads of a wave hit 64 different banks
#define IRS_NO_SET     0xFFFFFFFFu               // `set` of a row that does not exist

typedef float f4 __attribute__((ext_vector_type(4)));

// what the tile's rows are, in LDS
struct IrsTileRows {
    float2   hd[16];                             // the row's direct path h_d; +0 for a row that does not exist
    float    scale[16];                          // s_l; 0 for a row that does not exist
    uint32_t set[16], tap[16], ant[16];          // r or IRS_NO_SET, l, m
};

// thread i < 16 writes row i: row rho of set r, or with used = false a row that does not exist
__device__ __forceinline__ void irs_tile_row(IrsTileRows& t, uint32_t i, const IrsArgs& a, bool used, uint32_t r, uint32_t rho, uint2 key)
{
    const uint32_t L = a.n_taps, m = used ? rho / L : 0, l = used ? rho - m * L : 0;
    t.set[i] = used ? r : IRS_NO_SET;
    t.tap[i] = l;
    t.ant[i] = m;
    t.hd[i] = used ? irs_direct(a, m, r, l, key) : make_float2(0.0f, 0.0f);
    t.scale[i] = used ? a.scale[l] : 0.0f;
}

// the products of the chunk at n0 into `tile` [16][IRS_TILE_RS]: lane t of the 256 forms element n0 + (t & 63) of the rows
// (t >> 6) + 4 j into tile[row * IRS_TILE_RS + 2 * lane].  The caller's barriers stand before (the tables, the tile's last
// readers) and after it
__device__ __forceinline__ void irs_tile_form(float* tile, const IrsTileRows& t, const IrsArgs& a, uint32_t n0, uint32_t lane,
                                              uint32_t wave, uint2 key)
{
    const uint32_t n = n0 + lane;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t row = wave + 4 * j, r = t.set[row];
        float2 e = make_float2(0.0f, 0.0f);                     // no such row or element: the chain's zero terms
        if (r != IRS_NO_SET && n < a.n_elems) {
            const IrsElem el = irs_elem(a, t.ant[row], r, t.tap[row], n, key);
            e = ch_mul(el.a, el.b);
        }
        *reinterpret_cast<float2*>(&tile[row * IRS_TILE_RS + 2 * lane]) = e;
    }
}

}  // namespace wr
