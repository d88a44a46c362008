// Image metrics (nerf_amd_image_metrics, include/nerf_amd.h): the 11 x 11 Gaussian SSIM of Wang et al. over VALID positions and the whole-image
// MSE of fp32 (V, C, H, W) images, as fp64 per-view means.
//
// One workgroup (256 threads) takes one SEGMENT of one (view, channel) plane's SSIM map: IM_TW = 64 columns wide, up to IM_SEG_TILES = 8 tiles
// of IM_TH = 16 rows high, which it walks from the top, so that only the segment's first tile pays for the 10-row halo above it:
//   load   IM_TH new rows (the first time: the 10 halo rows) of the (64 + 10)-wide patches of x - 0.5 and y - 0.5 go to LDS (pixels outside
//          the image: 0, their outputs are masked).  The squared difference of the pixels that the segment OWNS is taken here, from the
//          registers that carry the load: a segment owns its 128 x 64 pixels, the last one of a column / row of segments also the 10-pixel
//          rim, so that every pixel of the plane counts once.
//   rows   the horizontal 11-tap pass of the five moments a, b, a^2, b^2, ab (a = x - 0.5, b = y - 0.5) of the new rows into
//          hb[moment][row & 31][column], a ring of 32 rows that always holds the 26 the tile needs: a thread takes TWO neighbouring columns
//          of one row, 12 taps of each input as six 8-byte LDS reads, the products formed once.
//   cols   the vertical pass of the tile: lane = column, wave w = rows 4w .. 4w+3, 14 rows x 5 moments read for four outputs.  The lanes of a
//          wave read 64 consecutive floats of one hb row, so the pass is free of bank conflicts at ANY row pitch; the pitch is IM_TW,
//          unpadded.  (The patches' pitch is IM_PP = 76, even, for the 8-byte reads of the row pass.)
//   then   the SSIM expression in fp32, the optional map store, and fp64 sums kept per lane over the segment; at its end lane -> wave
//          (shuffles) -> workgroup (LDS, fixed order) -> ONE (ssim sum, squared-difference sum) pair per workgroup in the workspace.
// image_metrics_final_kernel, one workgroup per view, adds the view's partials in a fixed order and divides by the counts.  No atomics anywhere:
// the result depends on the shapes alone, never on timing, and a view's bits do not depend on how many views share the call.
//
// Moments about 0.5: sigma_x^2 = <a^2> - <a>^2 holds for any offset, and |a| <= 0.5 on [0, 1] where |x| <= 1, so the cancellation in
// <x^2> - mu^2 works on terms up to four times smaller (and far smaller around mid-grey).  mu_x = 0.5 + <a>.  The bound that
// tests/image_metrics_ref.py derives follows this algorithm operation by operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "device_common.h"
#include "launchers.h"

namespace {

constexpr int IM_TH = NERF_AMD_IMAGE_METRICS_TILE_H, IM_TW = NERF_AMD_IMAGE_METRICS_TILE_W, IM_SEG_H = NERF_AMD_IMAGE_METRICS_SEGMENT_H;
constexpr int IM_SEG_TILES = IM_SEG_H / IM_TH;
constexpr int IM_K = 11, IM_HALO = IM_K - 1;
constexpr int IM_PW = IM_TW + IM_HALO;
constexpr int IM_PP = 76;                        // patch row pitch in floats: >= IM_PW, even
constexpr int IM_RING = 32;                      // rows of the hb ring: a power of two >= IM_TH + IM_HALO
constexpr int IM_ROWS_PER_WAVE = IM_TH / 4;      // four waves
static_assert(IM_TW == 64 && IM_TH == 16 && IM_ROWS_PER_WAVE == 4, "the thread maps below are written for a 16 x 64 tile and 256 threads");
static_assert(IM_PP >= IM_PW && IM_PP % 2 == 0 && IM_HALO <= IM_TH, "patch pitch; the halo rows are loaded through the tile's patch buffer");
static_assert(IM_RING >= IM_TH + IM_HALO && (IM_RING & (IM_RING - 1)) == 0 && IM_SEG_H % IM_TH == 0, "ring");

struct ImWindow { float g[IM_K]; };

// (p, q) summed over the workgroup into thread 0, in a fixed order
DEVINL void im_block_sum2(double& p, double& q, double* red) {
    p = wave_sum_d(p);
    q = wave_sum_d(q);
    const int w = (int)(threadIdx.x >> 6);
    if (lane_id() == 0) { red[2 * w] = p; red[2 * w + 1] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        p = ((red[0] + red[2]) + red[4]) + red[6];
        q = ((red[1] + red[3]) + red[5]) + red[7];
    }
}

// rows r_first .. r_first + nrows - 1 (nrows <= IM_TH), columns c0 .. c0 + IM_PW - 1 of the plane -> px, py (minus 0.5; 0 outside the image);
// sq += (x - y)^2 of the pixels with row < own_row_end and patch column < own_w
DEVINL void im_load_rows(float* px, float* py, const float* __restrict__ xp, const float* __restrict__ yp, int H, int W, int r_first, int nrows, int c0,
                         int own_row_end, int own_w, double& sq) {
    for (int i = (int)threadIdx.x; i < nrows * IM_PW; i += 256) {
        const int pr = i / IM_PW, pc = i - pr * IM_PW;
        const int r = r_first + pr, c = c0 + pc;
        float a = 0.0f, b = 0.0f;
        if (r < H && c < W) {
            const float xv = xp[(int64_t)r * W + c], yv = yp[(int64_t)r * W + c];
            a = xv - 0.5f;
            b = yv - 0.5f;
            if (r < own_row_end && pc < own_w) {
                const float d = xv - yv;
                sq += (double)d * (double)d;
            }
        }
        px[pr * IM_PP + pc] = a;
        py[pr * IM_PP + pc] = b;
    }
}

// hb[m][(ring_row0 + row) & 31][col] = sum_k g[k] * v_m[row][col + k], k ascending, for the nrows rows of px, py
DEVINL void im_row_pass(const float* px, const float* py, float (*hb)[IM_RING][IM_TW], int ring_row0, int nrows, const ImWindow& win) {
    for (int e = (int)threadIdx.x; e < nrows * (IM_TW / 2); e += 256) {
        const int row = e >> 5, col = (e & 31) * 2;
        float a[IM_K + 1], b[IM_K + 1];
        const float2* xr = reinterpret_cast<const float2*>(&px[row * IM_PP + col]);
        const float2* yr = reinterpret_cast<const float2*>(&py[row * IM_PP + col]);
#pragma unroll
        for (int k = 0; k < (IM_K + 1) / 2; ++k) {
            const float2 u = xr[k], v = yr[k];
            a[2 * k] = u.x; a[2 * k + 1] = u.y;
            b[2 * k] = v.x; b[2 * k + 1] = v.y;
        }
        float h[5][2];
#pragma unroll
        for (int m = 0; m < 5; ++m) { h[m][0] = 0.0f; h[m][1] = 0.0f; }
#pragma unroll
        for (int k = 0; k < IM_K + 1; ++k) {
            const float aa = a[k] * a[k], bb = b[k] * b[k], ab = a[k] * b[k];
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const int j = k - o;                         // tap of output column col + o
                if (j < 0 || j >= IM_K) continue;
                h[0][o] = __builtin_fmaf(win.g[j], a[k], h[0][o]);
                h[1][o] = __builtin_fmaf(win.g[j], b[k], h[1][o]);
                h[2][o] = __builtin_fmaf(win.g[j], aa, h[2][o]);
                h[3][o] = __builtin_fmaf(win.g[j], bb, h[3][o]);
                h[4][o] = __builtin_fmaf(win.g[j], ab, h[4][o]);
            }
        }
        const int rr = (ring_row0 + row) & (IM_RING - 1);
#pragma unroll
        for (int m = 0; m < 5; ++m) *reinterpret_cast<float2*>(&hb[m][rr][col]) = make_float2(h[m][0], h[m][1]);
    }
}

__global__ __launch_bounds__(256) void image_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ target, int H, int W, int strips,
                                                            int segs, ImWindow win, float* __restrict__ ssim_map, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float px[IM_TH * IM_PP];
    __shared__ __attribute__((aligned(16))) float py[IM_TH * IM_PP];
    __shared__ __attribute__((aligned(16))) float hb[5][IM_RING][IM_TW];
    __shared__ double red[8];

    const int tid = (int)threadIdx.x;
    const unsigned per_plane = (unsigned)strips * (unsigned)segs;
    const int64_t plane = (int64_t)(blockIdx.x / per_plane);
    const int part = (int)(blockIdx.x % per_plane);
    const int sy = part / strips, sx = part - sy * strips;
    const int R0 = sy * IM_SEG_H, c0 = sx * IM_TW;
    const int Ho = H - IM_HALO, Wo = W - IM_HALO;
    const float* __restrict__ xp = pred + plane * ((int64_t)H * W);
    const float* __restrict__ yp = target + plane * ((int64_t)H * W);
    const int rows_left = Ho - R0;                                               // >= 1
    const int n_tiles = rows_left >= IM_SEG_H ? IM_SEG_TILES : (rows_left + IM_TH - 1) / IM_TH;
    const int own_row_end = sy == segs - 1 ? H : R0 + IM_SEG_H, own_w = sx == strips - 1 ? IM_PW : IM_TW;

    const int col = lane_id(), rw = (tid >> 6) * IM_ROWS_PER_WAVE;
    const int oc = c0 + col;
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    double sq = 0.0, ss = 0.0;

    // the halo above the first tile
    im_load_rows(px, py, xp, yp, H, W, R0, IM_HALO, c0, own_row_end, own_w, sq);
    __syncthreads();
    im_row_pass(px, py, hb, 0, IM_HALO, win);
    __syncthreads();                                                             // (px, py are free again)

    for (int t = 0; t < n_tiles; ++t) {
        const int top = t * IM_TH;                                               // first output row of the tile within the segment = its first ring row
        im_load_rows(px, py, xp, yp, H, W, R0 + IM_HALO + top, IM_TH, c0, own_row_end, own_w, sq);
        __syncthreads();                                                         // (also: the previous tile's column pass is done with the ring rows written next)
        im_row_pass(px, py, hb, IM_HALO + top, IM_TH, win);
        __syncthreads();

        // ---- cols: four output rows per thread, tap j ascending for each
        float acc[5][IM_ROWS_PER_WAVE];
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int q = 0; q < IM_ROWS_PER_WAVE; ++q) acc[m][q] = 0.0f;
#pragma unroll
        for (int k = 0; k < IM_ROWS_PER_WAVE + IM_HALO; ++k) {
            const int rr = (top + rw + k) & (IM_RING - 1);
            float v[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) v[m] = hb[m][rr][col];
#pragma unroll
            for (int q = 0; q < IM_ROWS_PER_WAVE; ++q) {
                const int j = k - q;
                if (j < 0 || j >= IM_K) continue;
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[m][q] = __builtin_fmaf(win.g[j], v[m], acc[m][q]);
            }
        }

        // ---- SSIM of the four positions
#pragma unroll
        for (int q = 0; q < IM_ROWS_PER_WAVE; ++q) {
            const int orow = R0 + top + rw + q;
            const float ma = acc[0][q], mb = acc[1][q];
            const float mux = 0.5f + ma, muy = 0.5f + mb;
            const float vx = acc[2][q] - ma * ma, vy = acc[3][q] - mb * mb, cxy = acc[4][q] - ma * mb;
            const float num = (2.0f * (mux * muy) + C1) * (2.0f * cxy + C2);
            const float den = ((mux * mux + muy * muy) + C1) * ((vx + vy) + C2);
            const float s = num / den;
            if (orow < Ho && oc < Wo) {
                ss += (double)s;
                if (ssim_map) ssim_map[plane * ((int64_t)Ho * Wo) + (int64_t)orow * Wo + oc] = s;
            }
        }
    }

    im_block_sum2(ss, sq, red);
    if (tid == 0) { partial[2 * (int64_t)blockIdx.x] = ss; partial[2 * (int64_t)blockIdx.x + 1] = sq; }
}

// one workgroup per view: its n = C * segments partials, thread t taking t, t + 256, ... in order, then the fixed tree of im_block_sum2
__global__ __launch_bounds__(256) void image_metrics_final_kernel(const double* __restrict__ partial, int64_t n, double ssim_count, double mse_count,
                                                                  double* __restrict__ mse_out, double* __restrict__ ssim_out) {
    __shared__ double red[8];
    const double* pv = partial + 2 * n * (int64_t)blockIdx.x;
    double p = 0.0, q = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) { p += pv[2 * i]; q += pv[2 * i + 1]; }
    im_block_sum2(p, q, red);
    if (threadIdx.x == 0) {
        ssim_out[blockIdx.x] = p / ssim_count;
        mse_out[blockIdx.x] = q / mse_count;
    }
}

inline int64_t im_segments(int H, int W, int* strips, int* segs) {
    *strips = (W - IM_HALO + IM_TW - 1) / IM_TW;
    *segs = (H - IM_HALO + IM_SEG_H - 1) / IM_SEG_H;
    return (int64_t)*strips * *segs;
}

}  // namespace

int64_t nk::im_workgroups(int64_t V, int C, int H, int W) {
    int strips, segs;
    return V * C * im_segments(H, W, &strips, &segs);
}

// the 11 fp32 window weights: exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in fp64, each then rounded to fp32
void nk::im_window(float* g) {
    double w[IM_K], sum = 0.0;
    for (int i = 0; i < IM_K; ++i) { w[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += w[i]; }
    for (int i = 0; i < IM_K; ++i) g[i] = (float)(w[i] / sum);
}

int nk::im_image_metrics(const float* pred, const float* target, int64_t V, int C, int H, int W, double* mse_out, double* ssim_out, float* ssim_map, void* workspace,
                         hipStream_t st) {
    int strips, segs;
    const int64_t per_plane = im_segments(H, W, &strips, &segs);
    ImWindow win;
    im_window(win.g);
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(image_metrics_kernel, dim3((unsigned)(V * C * per_plane)), dim3(256), 0, st, pred, target, H, W, strips, segs, win, ssim_map, partial);
    hipLaunchKernelGGL(image_metrics_final_kernel, dim3((unsigned)V), dim3(256), 0, st, partial, (int64_t)C * per_plane, (double)C * (double)(H - IM_HALO) * (double)(W - IM_HALO),
                       (double)C * (double)H * (double)W, mse_out, ssim_out);
    return (int)hipGetLastError();
}
