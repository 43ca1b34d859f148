// kernels_distance.hip -- exact Euclidean distance fields over a lattice (mon_distance_transform, mon_scene_distance_lattice): per cell
// the least squared distance to an occupied cell and that cell's flat index.  Separable: one pass of k_distance_pass per axis (x, y, z), each the same
// minimisation along the lines of its axis,
//   out(p) = min over q of fl(fl(fl((float)(p - q) * step)^2) + in(q)),   site_out(p) = site_in(q*),  q* the lowest q at that minimum,
// which is what "candidates in ascending q, a strictly smaller one replaces" arrives at.  The x pass reads in(q) = 0 / +inf from the mask (fl(a^2 + 0) is
// a^2).  Every product and sum is a __fmul_rn / __fadd_rn: nothing is contracted, so the bits are those of the brute force over all pairs
// (tests/distance_reference.py).  k_distance_finish takes the root and applies max_dist.  No atomics, no scratch: equal arguments, equal bits.
#include <algorithm>
#include "distance_device.h"

namespace mon {

// The block shape (kDistTile, kDistOut), the block-wide maximum and an axis's lines and tile: distance_device.h, shared with the signed transform's seed pass.
struct DistPassArgs {
    const uint8_t* occ; uint32_t invert;                        // the x pass: the mask (a cell counts iff (occ != 0) != invert); else nullptr and ...
    const float* v_in; const int32_t* s_in;                     // ... the pass before: squared distance so far (+inf: none) and its site (-1)
    float* v_out; int32_t* s_out;
    uint32_t n, m, stride;                                      // cells per line, lines, elements between two cells of a line
    uint32_t cw, cs;                                            // line c begins at element (c / cw) * cs + c % cw
    uint32_t logR, rows_fast;                                   // the tile; rows_fast: consecutive threads take consecutive cells of a line (the x pass)
    float step;
};

// One pass.  Workgroup (line group cg, tile t_out of the lines): thread -> line c and rows r0 + o * dr of the tile, o < kDistOut.  With rows_fast the
// threads of a line are consecutive (the x pass: a line is contiguous in memory); otherwise consecutive threads take consecutive lines (the y and z passes:
// consecutive lines are consecutive i), so global loads and stores are coalesced either way.  An input tile in LDS is walked row by row by every thread at
// once: the threads of a line read one word (a broadcast), the lines of a wave consecutive words (rows_fast: lines padded by one word) -- no bank conflict.
// Candidates are compared by (value, site): a site's flat index grows with its cell's place along the pass's axis (the earlier axes vary faster, the later
// ones are the line's own), so "the lower site at an equal value" is "the lower q", in whatever order the tiles come.  That frees the order: the own tile
// first, then outward to the left while a tile can still matter, then to the right.  A tile dt tiles away holds no cell nearer than D = (dt - 1) R + 1
// cells, rounding is monotone, and in(q) >= 0, so every candidate of it is at least g = fl(fl(D step)^2): with B the largest best of the block, a left tile
// is skipped when g > B (an equal value at a lower q must still replace) and a right tile when g >= B, and so is everything beyond.  A staged tile without
// a finite cell is not walked (a +inf never replaces anything).  All of it keeps every bit of the unpruned definition.
__global__ void __launch_bounds__(256) k_distance_pass(DistPassArgs a) {
    __shared__ float s_v[kDistTile + 256];
    __shared__ int32_t s_s[kDistTile + 256];
    __shared__ float s_red[4];
    const uint32_t R = 1u << a.logR, C = kDistTile >> a.logR, nt = (a.n + R - 1u) / R;
    const uint32_t t_out = blockIdx.x % nt, cg = blockIdx.x / nt, tid = threadIdx.x;
    uint32_t c_loc, r0, dr, li0, lstep;
    if (a.rows_fast) { const uint32_t RL = R / kDistOut; c_loc = tid / RL; r0 = tid % RL; dr = RL; li0 = c_loc * (R + 1u); lstep = 1u; }
    else { c_loc = tid % C; r0 = tid / C; dr = 256u / C; li0 = c_loc; lstep = C; }
    const uint32_t c = cg * C + c_loc;
    const bool col_ok = c < a.m;
    const size_t base = col_ok ? (size_t)(c / a.cw) * a.cs + c % a.cw : 0;
    const uint32_t p0 = t_out * R + r0;                         // the thread's cells: rows p0 + o * dr of its line
    float best[kDistOut]; int32_t bsite[kDistOut];
#pragma unroll
    for (uint32_t o = 0; o < kDistOut; ++o) { best[o] = INFINITY; bsite[o] = INT32_MAX; }

    // tile t of the block's lines through LDS against the thread's cells; false: it held no finite cell and nothing changed
    auto tile = [&](uint32_t t) -> bool {
        __syncthreads();                                        // (the walk of the tile before is over)
        const uint32_t row_t = t * R;
        bool finite = false;
#pragma unroll
        for (uint32_t o = 0; o < kDistOut; ++o) {
            const uint32_t r = r0 + o * dr, q = row_t + r;
            float v = INFINITY; int32_t s = -1;
            if (col_ok && q < a.n) {
                const size_t g = base + (size_t)q * a.stride;
                if (a.occ) { const bool on = (a.occ[g] != 0) != (a.invert != 0u); v = on ? 0.f : INFINITY; s = on ? (int32_t)g : -1; }
                else { v = a.v_in[g]; s = a.s_in[g]; }
            }
            s_v[li0 + r * lstep] = v; s_s[li0 + r * lstep] = s;
            finite |= v < INFINITY;
        }
        if (!__syncthreads_or(finite)) return false;
        const uint32_t rows = min(R, a.n - row_t);
        for (uint32_t r = 0; r < rows; ++r) {
            const float v = s_v[li0 + r * lstep]; const int32_t s = s_s[li0 + r * lstep];
            const int32_t q = (int32_t)(row_t + r);
#pragma unroll
            for (uint32_t o = 0; o < kDistOut; ++o) {
                const float ax = __fmul_rn((float)((int32_t)(p0 + o * dr) - q), a.step);
                const float cand = __fadd_rn(__fmul_rn(ax, ax), v);
                if (cand < best[o] || (cand == best[o] && s < bsite[o])) { best[o] = cand; bsite[o] = s; }
            }
        }
        return true;
    };
    // the largest best among the block's cells of the lattice (cells past a line's end or past the last line do not count)
    auto bound = [&]() -> float {
        float x = 0.f;
#pragma unroll
        for (uint32_t o = 0; o < kDistOut; ++o) if (col_ok && p0 + o * dr < a.n) x = fmaxf(x, best[o]);
        return dist_block_max(x, s_red);
    };
    auto least = [&](uint32_t dt) -> float { const float ax = __fmul_rn((float)((dt - 1u) * R + 1u), a.step); return __fmul_rn(ax, ax); };

    tile(t_out);
    float B = bound();
    for (uint32_t dt = 1; dt <= t_out; ++dt) { if (least(dt) > B) break; if (tile(t_out - dt)) B = bound(); }
    for (uint32_t dt = 1; t_out + dt < nt; ++dt) { if (least(dt) >= B) break; if (tile(t_out + dt)) B = bound(); }

#pragma unroll
    for (uint32_t o = 0; o < kDistOut; ++o) {
        const uint32_t p = p0 + o * dr;
        if (col_ok && p < a.n) {
            const size_t g = base + (size_t)p * a.stride;
            a.v_out[g] = best[o]; a.s_out[g] = best[o] < INFINITY ? bsite[o] : -1;
        }
    }
}

// the mask of a density lattice: occupied iff !(sigma <= sigma_min) (a NaN or +inf sigma counts as occupied)
__global__ void __launch_bounds__(256) k_distance_mask(uint32_t n, const float* __restrict__ sigma, float sigma_min, uint8_t* __restrict__ occ) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) occ[i] = !(sigma[i] <= sigma_min) ? 1 : 0;
}

// dist = the correctly rounded root; where !(dist <= max_dist): dist = max_dist and no site.  nearest, nearest_owner (= owner[nearest], -1 without) may be
// nullptr.
__global__ void __launch_bounds__(256) k_distance_finish(uint32_t n, const float* __restrict__ d2, const int32_t* __restrict__ site, float max_dist,
        const int32_t* __restrict__ owner, float* __restrict__ dist, int32_t* __restrict__ nearest, int32_t* __restrict__ nearest_owner) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // (sqrtf: the IEEE root, v_sqrt_f32 with its residual correction -- __fsqrt_rn compiles to the bare instruction, which is 1 ulp off on some inputs)
    float d = sqrtf(d2[i]); int32_t s = site[i];
    if (!(d <= max_dist)) { d = max_dist; s = -1; }
    dist[i] = d;
    if (nearest) nearest[i] = s;
    if (nearest_owner) nearest_owner[i] = s >= 0 ? owner[s] : -1;
}

void launch_distance_mask(hipStream_t s, uint32_t n, const float* sigma, float sigma_min, uint8_t* occ) {
    hipLaunchKernelGGL(k_distance_mask, dim3((n + 255u) / 256u), dim3(256), 0, s, n, sigma, sigma_min, occ);
}
// one pass along axis ax: from the mask (occ; inverted or not), or with occ == nullptr from the values and sites of a pass before
static void distance_axis_launch(hipStream_t s, int ax, const Lattice& g, const uint8_t* occ, bool invert, const float* v_in, const int32_t* s_in, float* v_out,
        int32_t* s_out) {
    const DistAxis x = dist_axis(g, ax);
    DistPassArgs a{};
    if (occ) { a.occ = occ; a.invert = invert ? 1u : 0u; } else { a.v_in = v_in; a.s_in = s_in; }
    a.v_out = v_out; a.s_out = s_out;
    a.n = x.n; a.m = x.m; a.stride = x.stride; a.cw = x.cw; a.cs = x.cs; a.step = x.step; a.rows_fast = x.rows_fast; a.logR = x.logR;
    hipLaunchKernelGGL(k_distance_pass, dim3(x.blocks()), dim3(256), 0, s, a);
}
void launch_distance_axis(hipStream_t s, int ax, const Lattice& g, const float* v_in, const int32_t* s_in, float* v_out, int32_t* s_out) {
    distance_axis_launch(s, ax, g, nullptr, false, v_in, s_in, v_out, s_out);
}
// the three passes: occ (inverted or not) -> d2, site in v[0 .. n), site[0 .. n); v and site hold 2 n elements each (the passes alternate between the halves)
void launch_distance_passes(hipStream_t s, const uint8_t* occ, bool invert, const Lattice& g, float* v, int32_t* site) {
    const uint32_t n = (uint32_t)g.n();
    for (int ax = 0; ax < 3; ++ax) {
        const uint32_t in = ax == 1 ? 0u : n, out = ax == 1 ? n : 0u;       // x: mask -> low half; y: low -> high; z: high -> low
        distance_axis_launch(s, ax, g, ax == 0 ? occ : nullptr, invert, v + in, site + in, v + out, site + out);
    }
}
void launch_distance_finish(hipStream_t s, uint32_t n, const float* d2, const int32_t* site, float max_dist, const int32_t* owner, float* dist,
        int32_t* nearest, int32_t* nearest_owner) {
    hipLaunchKernelGGL(k_distance_finish, dim3((n + 255u) / 256u), dim3(256), 0, s, n, d2, site, max_dist, owner, dist, nearest, nearest_owner);
}

}  // namespace mon
