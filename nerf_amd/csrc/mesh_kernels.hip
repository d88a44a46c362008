// Iso-surface extraction (nerf_amd_mesh_count / nerf_amd_mesh_emit, include/nerf_amd.h): marching tetrahedra on the Kuhn split -- six
// tetrahedra per cell, one per order of the three axis steps from the cell's lowest corner to its highest -- of an fp32 lattice
// (nz, ny, nx).  The definition is in the header and, in fp64 and without any table, in tests/mesh_ref.py.
//
// Every lattice point p owns the 7 edges towards + (slot s: direction bits of s + 1).  One thread per point, 256 consecutive points (a
// TILE), four launches in two calls:
//   classify  reads the point's 8 cell corners (x-contiguous across the lanes; the neighbouring rows and planes come from the caches) and
//             stores ONE byte per point: bits 0..6 the slots whose ends lie on different sides of iso, bit 7 whether the point itself is
//             inside.  The inside flag of corner c of the cell that p names is then bit 7 ^ bit (c - 1): the later passes never read the
//             field to classify.  Per tile: the number of crossed slots (vertices) and of triangles, as two ints.
//   scan      one workgroup turns both tile arrays into exclusive prefixes (4096 tiles of each array per step in 16-byte accesses,
//             loaded one step ahead; wave scans + carries) and stores the totals as int64[2].
//   vertices  ranks the point's crossed slots -- tile prefix + wave scan + popcount below the slot --, stores the point's first vertex
//             id (prefix, int32: the id of (p, s) is prefix[p] + popc(byte[p] & ((1 << s) - 1))) and its vertices / normals.
//   faces     ranks the cell's triangles the same way and stores them in (cell, tetrahedron, triangle) order; a corner's vertex id
//             comes from the prefix and the byte of the edge's owner.
// No atomics: every output is a pure function of the input.  Every store of the two emit passes is guarded by the capacity the caller
// passed: a stale workspace or a wrong count gives wrong values, never a store out of bounds.
//
// The 16 cases of a tetrahedron per Kuhn tetrahedron (6 x 16 entries: the triangles as (owner corner, slot) pairs, winding resolved)
// are DERIVED at compile time, by the rule of the header and its exact integer orientation test: nothing is typed in.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "device_common.h"
#include "launchers.h"

namespace {

constexpr int MESH_TILE = 256;
constexpr int MESH_SCAN_GROUPS = 4;          // groups of 1024 tiles of each array per step of the scan
static_assert(MESH_SCAN_GROUPS * 1024 == NERF_AMD_MESH_SCAN_STEP_TILES, "the header and the tests name the scan's step");
constexpr int MESH_CLASSIFY_TILES = 8;       // consecutive tiles that one workgroup of the classify pass takes

// ---------------------------------------------------------------------------------------------------------------- the case table
// corner code of a cell: bit 0 = +x, bit 1 = +y, bit 2 = +z; the same bits name a slot's direction (slot = code - 1)
constexpr int MT_PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
constexpr int mt_corner(int t, int l) {
    return l == 0 ? 0 : l == 1 ? (1 << MT_PERM[t][0]) : l == 2 ? ((1 << MT_PERM[t][0]) | (1 << MT_PERM[t][1])) : 7;
}
// entry: bits 0..1 the triangle count; triangle k, corner j at bit 2 + 18 k + 6 j: owner corner code (3 bits) | slot << 3.
// ~0 marks a degenerate orientation test (never: the static_assert below).
constexpr uint64_t mt_entry(int t, int cs) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int l = 0; l < 4; ++l) {
        if ((cs >> l) & 1) in[ni++] = l; else out[no++] = l;
    }
    int tri[2][3][2] = {{{0, 0}, {0, 0}, {0, 0}}, {{0, 0}, {0, 0}, {0, 0}}};
    int ntri = 0;
    if (ni == 1 || ni == 3) {
        const int a = ni == 1 ? in[0] : out[0];
        const int* r = ni == 1 ? out : in;
        for (int j = 0; j < 3; ++j) { tri[0][j][0] = a; tri[0][j][1] = r[j]; }
        ntri = 1;
    } else if (ni == 2) {
        const int a = in[0], b = in[1], c = out[0], d = out[1];
        tri[0][0][0] = a; tri[0][0][1] = c; tri[0][1][0] = a; tri[0][1][1] = d; tri[0][2][0] = b; tri[0][2][1] = d;
        tri[1][0][0] = a; tri[1][0][1] = c; tri[1][1][0] = b; tri[1][1][1] = d; tri[1][2][0] = b; tri[1][2][1] = c;
        ntri = 2;
    }
    // (mean of the outside corners - mean of the inside corners) * ni * no, on the unit cell
    int dir[3] = {0, 0, 0};
    for (int ax = 0; ax < 3; ++ax) {
        int so = 0, si = 0;
        for (int l = 0; l < no; ++l) so += (mt_corner(t, out[l]) >> ax) & 1;
        for (int l = 0; l < ni; ++l) si += (mt_corner(t, in[l]) >> ax) & 1;
        dir[ax] = ni * so - no * si;
    }
    uint64_t enc = (uint64_t)ntri;
    for (int k = 0; k < ntri; ++k) {
        int p[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};          // twice the edge midpoints
        for (int j = 0; j < 3; ++j)
            for (int ax = 0; ax < 3; ++ax) p[j][ax] = ((mt_corner(t, tri[k][j][0]) >> ax) & 1) + ((mt_corner(t, tri[k][j][1]) >> ax) & 1);
        const int u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const int v[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        const int dot = (u[1] * v[2] - u[2] * v[1]) * dir[0] + (u[2] * v[0] - u[0] * v[2]) * dir[1] + (u[0] * v[1] - u[1] * v[0]) * dir[2];
        if (dot == 0) return ~(uint64_t)0;
        for (int j = 0; j < 3; ++j) {
            const int jj = (dot < 0 && j > 0) ? 3 - j : j;                         // swap the 2nd and 3rd entry
            const int e0 = tri[k][jj][0], e1 = tri[k][jj][1];
            const int lo = mt_corner(t, e0 < e1 ? e0 : e1), hi = mt_corner(t, e0 < e1 ? e1 : e0);
            enc |= (uint64_t)(lo | (((hi ^ lo) - 1) << 3)) << (2 + 18 * k + 6 * j);
        }
    }
    return enc;
}
struct MtTable { uint64_t e[6][16]; };
constexpr MtTable mt_make_table() {
    MtTable tb{};
    for (int t = 0; t < 6; ++t)
        for (int cs = 0; cs < 16; ++cs) tb.e[t][cs] = mt_entry(t, cs);
    return tb;
}
constexpr bool mt_table_ok(const MtTable& tb) {
    for (int t = 0; t < 6; ++t)
        for (int cs = 0; cs < 16; ++cs) {
            if (tb.e[t][cs] == ~(uint64_t)0) return false;
            const int n = __builtin_popcount(cs);
            if ((int)(tb.e[t][cs] & 3) != (n == 2 ? 2 : (n & 1))) return false;    // what mesh_cell_triangles counts
        }
    return true;
}
constexpr MtTable MT_HOST_TABLE = mt_make_table();
static_assert(mt_table_ok(MT_HOST_TABLE), "the orientation test is never degenerate; 1 / 2 / 1 triangles for 1 / 2 / 3 inside corners");
__constant__ MtTable MT_TABLE = mt_make_table();

// ---------------------------------------------------------------------------------------------------------------- device side
struct MeshArgs {
    const float* field;
    int nx, ny, nz;
    int64_t n;                       // nx * ny * nz < 2^31
    float iso, origin[3], spacing[3];
    uint8_t* byte;                   // per point: crossed slots | inside << 7
    int32_t* prefix;                 // per point: id of its first vertex
    int *tile_v, *tile_f;            // per tile: counts, after the scan exclusive prefixes
    int64_t n_tiles;
    uint64_t vcap, fcap;
    float *vertices, *normals;
    int32_t* faces;
};

DEVINL int mesh_wave() { return (int)(threadIdx.x >> 6); }
// inside flags of the 8 corners of the cell that a point names, from its byte (all 7 slots exist for a cell)
DEVINL unsigned mesh_corners_inside(unsigned byte) {
    const unsigned differs = (byte & 0x7fu) << 1;
    return (byte & 0x80u) ? (~differs & 0xffu) : differs;
}
DEVINL unsigned mesh_tet_case(unsigned in8, int t) {
    unsigned cs = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) cs |= ((in8 >> mt_corner(t, l)) & 1u) << l;
    return cs;
}
DEVINL int mesh_cell_triangles(unsigned in8) {
    int n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int c = __popc(mesh_tet_case(in8, t));
        n += c == 2 ? 2 : (c & 1);
    }
    return n;
}
// exclusive rank of this thread's `cnt` among the workgroup's, in thread order (wave scan, the four wave totals through LDS)
DEVINL int mesh_block_rank(int cnt, int* wave_total) {
    const int incl = wave_incl_scan_add(cnt);
    if (lane_id() == 63) wave_total[mesh_wave()] = incl;
    __syncthreads();
    int before = incl - cnt;
    for (int k = 0; k < mesh_wave(); ++k) before += wave_total[k];
    return before;
}

DEVINL void mesh_classify_tile(const MeshArgs& a, int64_t tile, int* wave_v, int* wave_f) {
    const int64_t p = tile * MESH_TILE + threadIdx.x;
    int nv = 0, nt = 0;
    if (p < a.n) {
        const unsigned up = (unsigned)p, row = up / (unsigned)a.nx;
        const int i = (int)(up - row * (unsigned)a.nx), k = (int)(row / (unsigned)a.ny), j = (int)(row - (unsigned)k * (unsigned)a.ny);
        const bool hx = i + 1 < a.nx, hy = j + 1 < a.ny, hz = k + 1 < a.nz;
        const int64_t sy = a.nx, sz = (int64_t)a.nx * a.ny;
        const float* f = a.field + p;
        const bool in0 = f[0] >= a.iso;                                        // (a NaN is outside)
        unsigned m = 0;
#pragma unroll
        for (int c = 1; c < 8; ++c) {
            const bool exists = (!(c & 1) || hx) && (!(c & 2) || hy) && (!(c & 4) || hz);
            if (exists) {
                const bool in = f[(c & 1) + ((c & 2) ? sy : 0) + ((c & 4) ? sz : 0)] >= a.iso;
                m |= (unsigned)(in != in0) << (c - 1);
            }
        }
        const unsigned byte = m | (in0 ? 0x80u : 0u);
        a.byte[p] = (uint8_t)byte;
        nv = __popc(m);
        if (hx && hy && hz) nt = mesh_cell_triangles(mesh_corners_inside(byte));
    }
    const int sv = wave_incl_scan_add(nv), sf = wave_incl_scan_add(nt);
    if (lane_id() == 63) { wave_v[mesh_wave()] = sv; wave_f[mesh_wave()] = sf; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.tile_v[tile] = (wave_v[0] + wave_v[1]) + (wave_v[2] + wave_v[3]);
        a.tile_f[tile] = (wave_f[0] + wave_f[1]) + (wave_f[2] + wave_f[3]);
    }
}
// A classify workgroup takes MESH_CLASSIFY_TILES consecutive tiles, one after the other: measured (profiles/mesh_extraction_summary.md),
// eight tiles per workgroup take 8 % off this pass, whose tiles all cost the same, and ADD 27-49 % to the emit passes, whose cost per
// tile follows the surface -- those take one tile per workgroup.
__global__ __launch_bounds__(256) void mesh_classify_kernel(MeshArgs a) {
    __shared__ int wave_v[4], wave_f[4];
    for (int it = 0; it < MESH_CLASSIFY_TILES; ++it) {
        const int64_t tile = blockIdx.x * (int64_t)MESH_CLASSIFY_TILES + it;
        if (tile >= a.n_tiles) break;                                          // (uniform)
        mesh_classify_tile(a, tile, wave_v, wave_f);
        __syncthreads();                                                       // the wave totals in LDS are free again
    }
}

// tiles -> exclusive prefixes in place (int32: a total of 2^31 or more is refused by the caller, from the int64 totals), totals -> counts[2]
__global__ __launch_bounds__(256) void mesh_scan_kernel(int* __restrict__ tile_v, int* __restrict__ tile_f, int64_t n_tiles_, int64_t* __restrict__ counts) {
    const int n_tiles = (int)n_tiles_;                                          // (< 2^23: 256 points per tile, fewer than 2^31 points)
    // Both arrays go through ONE loop of steps of MESH_SCAN_GROUPS x 1024 tiles.  In a group a thread owns FOUR consecutive tiles (one
    // 16-byte load, consecutive lanes on consecutive 16 bytes), a step's loads are issued one step ahead (they do not depend on the
    // carry), and all groups of a step share its two barriers: the single workgroup is bound by the latency of a step, not by its
    // 8 bytes per tile.  (The arrays are 256-byte aligned and padded to 256 bytes: a 16-byte access at a multiple of four stays inside.)
    __shared__ int wave_total[2][MESH_SCAN_GROUPS][4];
    const int lane = lane_id(), wv = mesh_wave();
    constexpr int G = MESH_SCAN_GROUPS;
    constexpr int STEP = G * 1024;
    int* const tiles[2] = {tile_v, tile_f};
    int4 cur[2][G], ahead[2][G] = {};
    auto load = [&](int base, int4 (&v)[2][G]) {
#pragma unroll
        for (int w = 0; w < 2; ++w)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int i0 = base + g * 1024 + (int)threadIdx.x * 4;
                int4 x = make_int4(0, 0, 0, 0);
                if (i0 < n_tiles) x = *reinterpret_cast<const int4*>(tiles[w] + i0);
                x.y = i0 + 1 < n_tiles ? x.y : 0;                                  // (beyond the last tile: padding, any content)
                x.z = i0 + 2 < n_tiles ? x.z : 0;
                x.w = i0 + 3 < n_tiles ? x.w : 0;
                v[w][g] = x;
            }
    };
    int64_t carry[2] = {0, 0};
    load(0, cur);
    for (int base = 0; base < n_tiles; base += STEP) {
        if (base + STEP < n_tiles) load(base + STEP, ahead);                       // (another range than the one written below)
        int sum[2][G], incl[2][G];
#pragma unroll
        for (int w = 0; w < 2; ++w)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                sum[w][g] = (cur[w][g].x + cur[w][g].y) + (cur[w][g].z + cur[w][g].w);
                incl[w][g] = wave_incl_scan_add(sum[w][g]);
                if (lane == 63) wave_total[w][g][wv] = incl[w][g];
            }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            int done = (int)(uint32_t)(uint64_t)carry[w];                          // of the groups before
            int step_total = 0;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                int before = 0, total = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) { before += k < wv ? wave_total[w][g][k] : 0; total += wave_total[w][g][k]; }
                const int i0 = base + g * 1024 + (int)threadIdx.x * 4;
                int4 out;
                out.x = done + before + (incl[w][g] - sum[w][g]);
                out.y = out.x + cur[w][g].x;
                out.z = out.y + cur[w][g].y;
                out.w = out.z + cur[w][g].z;
                if (i0 + 3 < n_tiles) {
                    *reinterpret_cast<int4*>(tiles[w] + i0) = out;
                } else {
                    if (i0 < n_tiles) tiles[w][i0] = out.x;
                    if (i0 + 1 < n_tiles) tiles[w][i0 + 1] = out.y;
                    if (i0 + 2 < n_tiles) tiles[w][i0 + 2] = out.z;
                }
                done += total;
                step_total += total;
            }
            carry[w] += step_total;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 2; ++w)
#pragma unroll
            for (int g = 0; g < G; ++g) cur[w][g] = ahead[w][g];
    }
    if (threadIdx.x == 0) { counts[0] = carry[0]; counts[1] = carry[1]; }
}

// (f[hi] - f[lo]) / (spacing * (hi - lo)) along one axis: central inside, one-sided on the lattice's faces
DEVINL float mesh_axis_gradient(const float* f, int idx, int n, int64_t stride, float spacing) {
    const int lo = idx > 0 ? -1 : 0, hi = idx + 1 < n ? 1 : 0;
    return (f[hi * stride] - f[lo * stride]) / (spacing * (float)(hi - lo));
}

DEVINL void mesh_vertex_tile(const MeshArgs& a, int64_t tile, int* wave_total) {
    const int64_t p = tile * MESH_TILE + threadIdx.x;
    const bool ok = p < a.n;
    const unsigned up = ok ? (unsigned)p : 0u, row = up / (unsigned)a.nx;
    const int i = (int)(up - row * (unsigned)a.nx), k = (int)(row / (unsigned)a.ny), j = (int)(row - (unsigned)k * (unsigned)a.ny);
    // the slots whose far end is in the lattice: what classify stored has no other bit; a stale workspace must not make this pass READ outside the field
    const unsigned exists = 0x7fu & (i + 1 < a.nx ? ~0u : ~0x55u) & (j + 1 < a.ny ? ~0u : ~0x66u) & (k + 1 < a.nz ? ~0u : ~0x78u);
    const unsigned m = ok ? (a.byte[p] & exists) : 0u;
    const int first = a.tile_v[tile] + mesh_block_rank(__popc(m), wave_total);
    if (!ok) return;
    a.prefix[p] = first;
    if (!m) return;
    const int64_t sy = a.nx, sz = (int64_t)a.nx * a.ny;
    const float* f = a.field + p;
    const float fa = f[0];
    float ga[3] = {0.0f, 0.0f, 0.0f};
    if (a.normals) {
        ga[0] = mesh_axis_gradient(f, i, a.nx, 1, a.spacing[0]);
        ga[1] = mesh_axis_gradient(f, j, a.ny, sy, a.spacing[1]);
        ga[2] = mesh_axis_gradient(f, k, a.nz, sz, a.spacing[2]);
    }
    int id = first;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        if (!((m >> s) & 1u)) continue;
        const int dx = (s + 1) & 1, dy = ((s + 1) >> 1) & 1, dz = ((s + 1) >> 2) & 1;
        const float* fq = f + (dx + (dy ? sy : 0) + (dz ? sz : 0));
        float t = (a.iso - fa) / (fq[0] - fa);
        t = (t - t == 0.0f) ? fminf(fmaxf(t, 0.0f), 1.0f) : 0.5f;            // non-finite -> 0.5
        const uint64_t at = (uint64_t)(int64_t)id;                            // (a negative id of a stale workspace is refused too)
        if (at < a.vcap) {
            float* v = a.vertices + 3 * at;
            v[0] = a.origin[0] + a.spacing[0] * (dx ? (float)i + t : (float)i);
            v[1] = a.origin[1] + a.spacing[1] * (dy ? (float)j + t : (float)j);
            v[2] = a.origin[2] + a.spacing[2] * (dz ? (float)k + t : (float)k);
            if (a.normals) {
                const float gb0 = mesh_axis_gradient(fq, i + dx, a.nx, 1, a.spacing[0]);
                const float gb1 = mesh_axis_gradient(fq, j + dy, a.ny, sy, a.spacing[1]);
                const float gb2 = mesh_axis_gradient(fq, k + dz, a.nz, sz, a.spacing[2]);
                const float w0 = 1.0f - t;
                const float vx = w0 * ga[0] + t * gb0, vy = w0 * ga[1] + t * gb1, vz = w0 * ga[2] + t * gb2;
                const float len = sqrtf((vx * vx + vy * vy) + vz * vz);
                const bool good = len > 0.0f && len - len == 0.0f;            // zero or non-finite -> (0, 0, 0)
                float* nn = a.normals + 3 * at;
                nn[0] = good ? -(vx / len) : 0.0f;
                nn[1] = good ? -(vy / len) : 0.0f;
                nn[2] = good ? -(vz / len) : 0.0f;
            }
        }
        ++id;
    }
}
__global__ __launch_bounds__(256) void mesh_vertex_kernel(MeshArgs a) {
    __shared__ int wave_total[4];
    mesh_vertex_tile(a, blockIdx.x, wave_total);
}

DEVINL void mesh_face_tile(const MeshArgs& a, int64_t tile, int* wave_total) {
    const int64_t p = tile * MESH_TILE + threadIdx.x;
    unsigned in8 = 0;
    int cnt = 0;
    if (p < a.n) {
        const unsigned up = (unsigned)p, row = up / (unsigned)a.nx;
        const int i = (int)(up - row * (unsigned)a.nx), k = (int)(row / (unsigned)a.ny), j = (int)(row - (unsigned)k * (unsigned)a.ny);
        if (i + 1 < a.nx && j + 1 < a.ny && k + 1 < a.nz) {
            in8 = mesh_corners_inside(a.byte[p]);
            cnt = mesh_cell_triangles(in8);
        }
    }
    int at = a.tile_f[tile] + mesh_block_rank(cnt, wave_total);
    if (!cnt) return;
    const int64_t sy = a.nx, sz = (int64_t)a.nx * a.ny;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const uint64_t e = MT_TABLE.e[t][mesh_tet_case(in8, t)];
        const int ntri = (int)(e & 3u);
        for (int k = 0; k < ntri; ++k, ++at) {
            const uint64_t slot = (uint64_t)(int64_t)at;
            if (slot >= a.fcap) continue;
            int32_t* out = a.faces + 3 * slot;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const unsigned c = (unsigned)(e >> (2 + 18 * k + 6 * j)) & 63u;
                const int64_t q = p + (int64_t)(c & 1u) + ((c & 2u) ? sy : 0) + ((c & 4u) ? sz : 0);      // the edge's owner: a corner of this cell
                out[j] = a.prefix[q] + __popc((unsigned)a.byte[q] & ((1u << (c >> 3)) - 1u));
            }
        }
    }
}
__global__ __launch_bounds__(256) void mesh_face_kernel(MeshArgs a) {
    __shared__ int wave_total[4];
    mesh_face_tile(a, blockIdx.x, wave_total);
}

struct MeshWs { uint8_t* byte; int32_t* prefix; int *tile_v, *tile_f; int64_t n_tiles; size_t bytes; };
inline MeshWs mesh_ws(int64_t n, void* workspace) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    MeshWs w;
    w.n_tiles = (n + MESH_TILE - 1) / MESH_TILE;
    char* at = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    w.byte = reinterpret_cast<uint8_t*>(at); at += up((size_t)n);
    w.prefix = reinterpret_cast<int32_t*>(at); at += up((size_t)n * 4);
    w.tile_v = reinterpret_cast<int*>(at); at += up((size_t)w.n_tiles * 4);
    w.tile_f = reinterpret_cast<int*>(at);
    w.bytes = up((size_t)n) + up((size_t)n * 4) + 2 * up((size_t)w.n_tiles * 4) + 256;     // + the alignment slack
    return w;
}
inline unsigned mesh_grid(const MeshWs& w, int tiles) { return (unsigned)((w.n_tiles + tiles - 1) / tiles); }
inline MeshArgs mesh_args(const float* field, int nx, int ny, int nz, float iso, const MeshWs& w) {
    MeshArgs a{};
    a.field = field; a.nx = nx; a.ny = ny; a.nz = nz; a.n = (int64_t)nx * ny * nz; a.iso = iso;
    a.byte = w.byte; a.prefix = w.prefix; a.tile_v = w.tile_v; a.tile_f = w.tile_f; a.n_tiles = w.n_tiles;
    return a;
}

}  // namespace

size_t nk::mesh_workspace_bytes(int nx, int ny, int nz) { return mesh_ws((int64_t)nx * ny * nz, nullptr).bytes; }

int nk::mesh_count(const float* field, int nx, int ny, int nz, float iso, int64_t* counts_dev, void* workspace, hipStream_t st) {
    const MeshWs w = mesh_ws((int64_t)nx * ny * nz, workspace);
    const MeshArgs a = mesh_args(field, nx, ny, nz, iso, w);
    hipLaunchKernelGGL(mesh_classify_kernel, dim3(mesh_grid(w, MESH_CLASSIFY_TILES)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(256), 0, st, w.tile_v, w.tile_f, w.n_tiles, counts_dev);
    return (int)hipGetLastError();
}

int nk::mesh_emit(const float* field, int nx, int ny, int nz, float iso, const float* origin, const float* spacing, void* workspace, int64_t vertex_capacity,
                  int64_t face_capacity, float* vertices, float* normals, int32_t* faces, hipStream_t st) {
    const MeshWs w = mesh_ws((int64_t)nx * ny * nz, workspace);
    MeshArgs a = mesh_args(field, nx, ny, nz, iso, w);
    for (int c = 0; c < 3; ++c) { a.origin[c] = origin[c]; a.spacing[c] = spacing[c]; }
    a.vcap = (uint64_t)vertex_capacity; a.fcap = (uint64_t)face_capacity;
    a.vertices = vertices; a.normals = normals; a.faces = faces;
    hipLaunchKernelGGL(mesh_vertex_kernel, dim3(mesh_grid(w, 1)), dim3(256), 0, st, a);      // (also: the per-point prefix that the faces read)
    hipLaunchKernelGGL(mesh_face_kernel, dim3(mesh_grid(w, 1)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}
