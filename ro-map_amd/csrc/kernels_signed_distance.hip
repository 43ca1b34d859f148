// kernels_signed_distance.hip -- signed, sub-cell distance fields over a lattice (mon_signed_distance_transform, mon_scene_signed_distance_lattice,
// mon_scene_signed_dist_field; the rule: include/mon_core.h).  The surface is the level set val = iso, placed INSIDE the lattice edges:
// an edge whose two cells differ in `inside` carries a crossing at the fraction f = fl(fl(iso - v0) / fl(v1 - v0)) of its length (0.5 when that is not in
// [0, 1]: infinite and NaN values).  Per cell: the least squared distance to a crossing, over the edges of all three axes, the edge that gives it
// (3 * flat(q) + axis), and the sign from the cell's own side.  Separable, as kernels_distance.hip: per axis a one chain of three passes --
//   k_surface_line_pass along a:  u(p) = min over the crossing edges q of the line of fl(t t),  t = fl(fl((float)(p - q) - f) * step_a)
//   k_distance_pass along the other two axes in ascending order, from values (launch_distance_axis)
// -- and k_signed_finish takes the least of the three chains, the root, the cut at max_dist, the sign and the owner.  Every product, sum and quotient is
// one separately rounded fp32 operation: the bits are those of the brute force over all (cell, crossing) pairs (tests/signed_distance_reference.py).
// Sites.  k_distance_pass compares candidates by (value, site) and prunes on "the lower site at an equal value is the lower q".  That holds when the axes
// passed earlier vary faster in the site than the pass's own.  Chain x (x, y, z) has it with the flat index.  Chains y (y, x, z) and z (z, x, y) do not,
// so inside a chain an edge is carried as 3 * code + a with the CODE of its lower cell, the cell's index with the chain's seed axis fastest:
//   chain y: code = (k * nx + i) * ny + j;   chain z: code = (j * nx + i) * nz + k;   chain x: the flat index.
// Every pass then sees codes that grow with q, "ascending q, a strictly smaller one replaces" is what all nine passes compute whatever they prune, and
// the finish turns the winner's code back into the flat index.  No atomics, no scratch, no inline assembly: equal arguments, equal bits.
#include "distance_device.h"

namespace mon {

struct SurfacePassArgs {
    const float* val; const uint8_t* ins;                       // the values and each cell's side (1: inside)
    const float* iso_p; float iso;                              // the level: iso_p[0] on the device (the scene routes form it there), nullptr: iso
    float* v_out; int32_t* s_out;
    uint32_t n, m, stride;                                      // cells per line, lines, elements between two cells of a line
    uint32_t cw, cs;                                            // line c begins at element (c / cw) * cs + c % cw
    uint32_t logR, rows_fast;
    float step;
    uint32_t nx, ny;                                            // the lattice (a line's first cell -> its coordinates)
    uint32_t ei, ej, ek, axis;                                  // the chain's code: i * ei + j * ej + k * ek; the seed axis
};

// The seed pass.  k_distance_pass's block (distance_device.h; the thread map, the LDS layout and the walk are that kernel's) with another candidate: tile t
// of a line stages, for each of its edges q (cells q and q + 1 of the line, q + 1 < n), the crossing's fraction f, or -1 where the two cells lie on one
// side; both are formed while staging from val and ins at q and q + 1 (the second load falls into the line the neighbouring thread fetches).  The site is
// not staged: it is 3 (code0 + q e_a) + a, one multiply-add per row.  Candidates are compared by (value, site) as there, and the code grows with q, so
// the order of the tiles is free: the own tile, then to the left, then to the right.  The crossing of edge q lies in [q, q + 1]: a tile dt tiles to the
// LEFT holds nothing nearer than (dt - 1) R cells (its last edge ends on the own tile's first cell), one to the RIGHT nothing nearer than (dt - 1) R + 1,
// fl(x - f) and the products are monotone, so with B the largest best of the block a left tile is skipped when g > B (an equal value at a lower q must
// still replace) and a right tile when g >= B, and so is everything beyond.  A staged tile without a crossing is not walked.
__global__ void __launch_bounds__(256) k_surface_line_pass(SurfacePassArgs a) {
    __shared__ float s_f[kDistTile + 256];
    __shared__ float s_red[4];
    const uint32_t R = 1u << a.logR, C = kDistTile >> a.logR, nt = (a.n + R - 1u) / R;
    const uint32_t t_out = blockIdx.x % nt, cg = blockIdx.x / nt, tid = threadIdx.x;
    uint32_t c_loc, r0, dr, li0, lstep;
    if (a.rows_fast) { const uint32_t RL = R / kDistOut; c_loc = tid / RL; r0 = tid % RL; dr = RL; li0 = c_loc * (R + 1u); lstep = 1u; }
    else { c_loc = tid % C; r0 = tid / C; dr = 256u / C; li0 = c_loc; lstep = C; }
    const uint32_t c = cg * C + c_loc;
    const bool col_ok = c < a.m;
    const uint32_t base = col_ok ? (c / a.cw) * a.cs + c % a.cw : 0u;              // (n <= 2^22: a flat index fits 32 bits, three times it too)
    const uint32_t code0 = (base % a.nx) * a.ei + ((base / a.nx) % a.ny) * a.ej + (base / (a.nx * a.ny)) * a.ek;
    const uint32_t ea = a.axis == 0u ? a.ei : a.axis == 1u ? a.ej : a.ek;
    const uint32_t p0 = t_out * R + r0;                         // the thread's cells: rows p0 + o * dr of its line
    const float iso = a.iso_p ? a.iso_p[0] : a.iso;
    float best[kDistOut]; int32_t bsite[kDistOut];
#pragma unroll
    for (uint32_t o = 0; o < kDistOut; ++o) { best[o] = INFINITY; bsite[o] = INT32_MAX; }

    // the edges of tile t of the block's lines through LDS against the thread's cells; false: it held no crossing and nothing changed
    auto tile = [&](uint32_t t) -> bool {
        __syncthreads();                                        // (the walk of the tile before is over)
        const uint32_t row_t = t * R;
        bool any = false;
#pragma unroll
        for (uint32_t o = 0; o < kDistOut; ++o) {
            const uint32_t r = r0 + o * dr, q = row_t + r;
            float f = -1.f;
            if (col_ok && q + 1u < a.n) {
                const uint32_t g = base + q * a.stride, g1 = g + a.stride;
                if ((a.ins[g] != 0) != (a.ins[g1] != 0)) {
                    const float v0 = a.val[g], v1 = a.val[g1];
                    f = __fdiv_rn(__fsub_rn(iso, v0), __fsub_rn(v1, v0));
                    if (!(f >= 0.f && f <= 1.f)) f = 0.5f;
                }
            }
            s_f[li0 + r * lstep] = f;
            any |= f >= 0.f;
        }
        if (!__syncthreads_or(any)) return false;
        const uint32_t rows = min(R, a.n - row_t);
        for (uint32_t r = 0; r < rows; ++r) {
            const float f = s_f[li0 + r * lstep];
            const int32_t q = (int32_t)(row_t + r);
            const int32_t s = f >= 0.f ? (int32_t)(3u * (code0 + (uint32_t)q * ea) + a.axis) : -1;
#pragma unroll
            for (uint32_t o = 0; o < kDistOut; ++o) {
                const float t1 = __fmul_rn(__fsub_rn((float)((int32_t)(p0 + o * dr) - q), f), a.step);
                const float cand = f >= 0.f ? __fmul_rn(t1, t1) : INFINITY;
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
    auto least = [&](uint32_t cells) -> float { const float ax = __fmul_rn((float)cells, a.step); return __fmul_rn(ax, ax); };

    tile(t_out);
    float B = bound();
    for (uint32_t dt = 1; dt <= t_out; ++dt) { if (least((dt - 1u) * R) > B) break; if (tile(t_out - dt)) B = bound(); }
    for (uint32_t dt = 1; t_out + dt < nt; ++dt) { if (least((dt - 1u) * R + 1u) >= B) break; if (tile(t_out + dt)) B = bound(); }

#pragma unroll
    for (uint32_t o = 0; o < kDistOut; ++o) {
        const uint32_t p = p0 + o * dr;
        if (col_ok && p < a.n) {
            const uint32_t g = base + p * a.stride;
            a.v_out[g] = best[o]; a.s_out[g] = best[o] < INFINITY ? bsite[o] : -1;
        }
    }
}

// The interpolated values of a density lattice: val = logf(sigma) and iso = logf(sigma_min) (use_log), else sigma and sigma_min themselves; the side is
// taken from sigma either way, ins = !(sigma <= sigma_min) (k_distance_mask's bit).  val (nullptr: the caller's values are used as they are) and iso_out
// (nullptr: not asked for) are written by the same function, so a level that equals a value keeps equal bits.
__global__ void __launch_bounds__(256) k_signed_values(uint32_t n, const float* __restrict__ sigma, float sigma_min, uint32_t use_log, float* __restrict__ val,
        uint8_t* __restrict__ ins, float* __restrict__ iso_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0u && iso_out) iso_out[0] = use_log ? logf(sigma_min) : sigma_min;
    if (i >= n) return;
    const float x = sigma[i];
    ins[i] = !(x <= sigma_min) ? 1 : 0;
    if (val) val[i] = use_log ? logf(x) : x;
}

// The least of the three chains (x, then y, then z; a strictly smaller one replaces and brings its edge), the correctly rounded root, the cut (where
// !(d <= max_dist): d = max_dist and no edge), the sign.  w, site: the chains' results, [3][n] with `pitch` elements between two chains.  nearest_edge =
// 3 * flat(q) + a, the chain's code turned back; nearest_owner = owner[] at the inside end of that edge.  Both may be nullptr.
__global__ void __launch_bounds__(256) k_signed_finish(uint32_t n, uint32_t nx, uint32_t ny, uint32_t nz, const float* __restrict__ w,
        const int32_t* __restrict__ site, uint32_t pitch, const uint8_t* __restrict__ ins, float max_dist, const int32_t* __restrict__ owner,
        float* __restrict__ sdist, int32_t* __restrict__ nearest_edge, int32_t* __restrict__ nearest_owner) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float d2 = w[i]; int32_t s = site[i]; uint32_t chain = 0u;
    if (w[pitch + i] < d2) { d2 = w[pitch + i]; s = site[pitch + i]; chain = 1u; }
    if (w[2u * pitch + i] < d2) { d2 = w[2u * pitch + i]; s = site[2u * pitch + i]; chain = 2u; }
    // (sqrtf: the IEEE root, as k_distance_finish takes it)
    float d = sqrtf(d2);
    if (!(d <= max_dist)) { d = max_dist; s = -1; }
    const bool in = ins[i] != 0;
    sdist[i] = in ? -d : d;
    int32_t edge = -1, own = -1;
    if (s >= 0) {
        const uint32_t a = (uint32_t)s % 3u, code = (uint32_t)s / 3u;
        uint32_t flat = code;
        if (chain == 1u) { const uint32_t j = code % ny, r = code / ny; flat = ((r / nx) * ny + j) * nx + r % nx; }
        else if (chain == 2u) { const uint32_t k = code % nz, r = code / nz; flat = (k * ny + r / nx) * nx + r % nx; }
        edge = (int32_t)(3u * flat + a);
        if (nearest_owner) { const uint32_t other = flat + (a == 0u ? 1u : a == 1u ? nx : nx * ny); own = owner[ins[flat] != 0 ? flat : other]; }
    }
    if (nearest_edge) nearest_edge[i] = edge;
    if (nearest_owner) nearest_owner[i] = own;
}

void launch_signed_values(hipStream_t s, uint32_t n, const float* sigma, float sigma_min, bool use_log, float* val, uint8_t* ins, float* iso_out) {
    hipLaunchKernelGGL(k_signed_values, dim3((n + 255u) / 256u), dim3(256), 0, s, n, sigma, sigma_min, use_log ? 1u : 0u, val, ins, iso_out);
}
// The nine passes (the level: iso_p[0] on the device, or with iso_p == nullptr iso): chain a's result in v[a n .. (a + 1) n) and site[a n ..); v and site hold 4 n elements (the fourth part is the passes' other half)
void launch_signed_passes(hipStream_t s, const float* val, const uint8_t* ins, const float* iso_p, float iso, const Lattice& g, float* v, int32_t* site) {
    const uint32_t nx = (uint32_t)g.nx, ny = (uint32_t)g.ny, nz = (uint32_t)g.nz, n = nx * ny * nz;
    const uint32_t code[3][3] = { { 1u, nx, nx * ny }, { ny, 1u, nx * ny }, { nz, nx * nz, 1u } };
    for (int c = 0; c < 3; ++c) {
        const DistAxis x = dist_axis(g, c);
        float* const v_own = v + (size_t)c * n; float* const v_tmp = v + 3 * (size_t)n;
        int32_t* const s_own = site + (size_t)c * n; int32_t* const s_tmp = site + 3 * (size_t)n;
        SurfacePassArgs a{};
        a.val = val; a.ins = ins; a.iso_p = iso_p; a.iso = iso; a.v_out = v_own; a.s_out = s_own;
        a.n = x.n; a.m = x.m; a.stride = x.stride; a.cw = x.cw; a.cs = x.cs; a.logR = x.logR; a.rows_fast = x.rows_fast; a.step = x.step;
        a.nx = nx; a.ny = ny; a.ei = code[c][0]; a.ej = code[c][1]; a.ek = code[c][2]; a.axis = (uint32_t)c;
        hipLaunchKernelGGL(k_surface_line_pass, dim3(x.blocks()), dim3(256), 0, s, a);
        const int b0 = c == 0 ? 1 : 0, b1 = c == 2 ? 1 : 2;    // the other two axes, ascending: own -> the other half -> own
        launch_distance_axis(s, b0, g, v_own, s_own, v_tmp, s_tmp);
        launch_distance_axis(s, b1, g, v_tmp, s_tmp, v_own, s_own);
    }
}
void launch_signed_finish(hipStream_t s, const Lattice& g, const float* v, const int32_t* site, const uint8_t* ins, float max_dist, const int32_t* owner,
        float* sdist, int32_t* nearest_edge, int32_t* nearest_owner) {
    const uint32_t n = (uint32_t)g.n();
    hipLaunchKernelGGL(k_signed_finish, dim3((n + 255u) / 256u), dim3(256), 0, s, n, (uint32_t)g.nx, (uint32_t)g.ny, (uint32_t)g.nz, v, site, n, ins, max_dist,
            owner, sdist, nearest_edge, nearest_owner);
}

}  // namespace mon
