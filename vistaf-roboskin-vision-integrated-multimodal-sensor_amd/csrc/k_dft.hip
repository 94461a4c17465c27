// Side-band demodulation as a pruned DFT (shape_ftp.py:857-997).
//
// The reference reflect-pads the n x n crop to N x N, takes fft2, keeps a (2*bw+1)^2 patch around the
// (locked) carrier, windows it, moves it to DC, takes ifft2, applies a sub-bin ramp and crops.  Only
// ph*pw (<= 21x21) spectral bins are ever used, so both transforms are computed directly:
//   forward  patch = win . ( Ey[ph x h] . (iw - mu)[h x w] . Ex[w x pw] )       (reflect pad folded into Ex/Ey)
//   inverse  field = Gy[h x ph] . patch[ph x pw] . Gx[pw x w]                   (crop, ramp, 1/N^2 folded in)
// Everything between the float32 input plane and the float32 results (amplitude, wrapped phase difference) is
// float64: float64 twiddles built on the host, float64 fused multiply-adds, float64 patch / field.  That is the
// arithmetic of the reference under NumPy < 2 (fft2 of a float32 array runs in complex128; the sub-bin ramp and
// cdef * conj(cref) are complex128 under every NumPy), to ~1e-15 relative -- so amplitude and wrapped phase round
// to the same float32 as a complex128 NumPy transform's (what the parity tests compare with) and every threshold downstream of them
// (quality >= p25) sees the same plane.  Tables may be per frame (tab_stride != 0: the uncached-pair mode, where
// every sample carries its own carrier) or shared by the batch (0).
#include <algorithm>
#include "kernels.hpp"
#include "cgemm_mfma.hpp"

namespace vf {

__device__ inline void cmac(double &ar, double &ai, double er, double ei, double vr, double vi)
{
    ar = fma(er, vr, ar); ar = fma(-ei, vi, ar);
    ai = fma(er, vi, ai); ai = fma(ei, vr, ai);
}

// stage 1 as a float64 GEMM on the matrix cores: C[row = (b, y)][n] = sum_x V[row][x] * E[x][n], n = 0..2*pw-1 (real parts of the pw bins,
// then their imaginary parts), with v_mfma_f64_16x16x4_f64: A[i = lane & 15][k = lane >> 4] = V, B[k = lane >> 4][j = lane & 15] = E,
// D[row = (lane >> 4) + 4 * reg][col = lane & 15].  One wave owns a strip of 16 image rows and all column tiles (<= DFT_MAXT at a time);
// operands come straight from global memory / L2 (the table is 2 * pw * w doubles), one element per lane and k-step.  This is the only dense
// contraction of the path; float64 keeps the accumulation the parity of the demodulated field relies on.
// The rows form nseg segments of seg_rows rows, each with its own table (Ex_all + seg * ex_stride): one segment of B * h rows for a shared
// table, one per frame for per-frame tables (pair mode).  Strips start at each segment's first row, so a strip never mixes two tables, at
// any h.  An output row depends only on its own input row and the table (the same k-steps in the same order), not on the strip it sits
// in: a pair sample gives the bits of a session built on its reference.
constexpr int DFT_MAXT = 4;            // column tiles (16 columns each) accumulated per pass over x
__global__ __launch_bounds__(256) void k_dft_fwd1_mfma(const float *__restrict__ iw, const float *__restrict__ mu, const double2 *__restrict__ Ex_all,
                                                       size_t ex_stride, double2 *__restrict__ T, int h, int w, int pw, int seg_rows, int nseg)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int sps = (seg_rows + 15) / 16;                       // strips per segment
    const int strip = blockIdx.x * 4 + wid;
    if (strip >= nseg * sps) return;
    const int seg = strip / sps;
    const int row0 = seg * seg_rows + (strip - seg * sps) * 16;
    const int row_end = (seg + 1) * seg_rows;                   // one past the segment's last row
    const int r = lane & 15, kk = lane >> 4;
    const int grow = min(row0 + r, row_end - 1);                // rows past the segment repeat its last one (never stored)
    const double *E = (const double *)(Ex_all + (size_t)seg * ex_stride);
    const float *src = iw + (size_t)grow * w;
    const float m = mu ? mu[grow / h] : 0.f;
    const int ncol = 2 * pw, ntile = (ncol + 15) / 16;
    for (int t0 = 0; t0 < ntile; t0 += DFT_MAXT) {
        v4f64 acc[DFT_MAXT];
        int eoff[DFT_MAXT];                                     // offset of this lane's column inside one table row (doubles), -1: padding column
#pragma unroll
        for (int t = 0; t < DFT_MAXT; t++) {
            acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
            const int n = (t0 + t) * 16 + r;
            eoff[t] = (t0 + t < ntile && n < ncol) ? (n < pw ? 2 * n : 2 * (n - pw) + 1) : -1;
        }
        for (int x0 = 0; x0 < w; x0 += 4) {
            const int x = x0 + kk;
            const bool in = x < w;
            const double a = in ? (double)__fsub_rn(src[in ? x : 0], m) : 0.0;
            double bv[DFT_MAXT];
#pragma unroll
            for (int t = 0; t < DFT_MAXT; t++) bv[t] = (in && eoff[t] >= 0) ? E[(size_t)x * (2 * pw) + eoff[t]] : 0.0;
#pragma unroll
            for (int t = 0; t < DFT_MAXT; t++)
                if (t0 + t < ntile) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv[t], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < DFT_MAXT; t++) {
            if (eoff[t] < 0) continue;
            const int n = (t0 + t) * 16 + r, c = n < pw ? n : n - pw;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int row = row0 + kk + 4 * q;
                if (row < row_end) ((double *)(T + (size_t)row * pw + c))[n < pw ? 0 : 1] = acc[t][q];
            }
        }
    }
}

// What of the demodulation runs on the staged kernels (Tiers::dft_staged) at this shape: DFT_STAGED_FWD1 stage 1 as k_dft_fwd1_staged,
// DFT_STAGED_INV2 stage 4 as k_dft_inv2_staged.  The limits are those of the kernels' LDS images and of the loads a thread issues per chunk;
// frame size and table mode exclude nothing (the table goes in chunks, a workgroup stays inside one segment).  Every other shape, and
// stages 2 and 3, take the kernels that read global memory.
constexpr int FWD1_MAXPW = 24;                                   // 2 pw <= 48 columns: three tiles, one pass; three table loads per thread and chunk
constexpr int INV2_MAXPH = 22;                                   // 2 KB of LDS per row + 4 KB: 48 KB; 6 staging loads per thread
int dft_staged_fits(int h, int w, int ph, int pw, bool per_frame_tables)
{
    (void)per_frame_tables;
    if (h < 1 || w < 1 || ph < 1 || pw < 1) return 0;
    return (pw <= FWD1_MAXPW ? DFT_STAGED_FWD1 : 0) | (ph <= INV2_MAXPH ? DFT_STAGED_INV2 : 0);
}

// stage 1 with its operands staged in LDS (Tiers::dft_staged, patches dft_staged_fits takes: all column tiles in one pass).  A workgroup owns
// four strips of ONE segment (its four waves; the grid is per segment, so no workgroup sees two tables) and walks x in chunks of FWD1_XC
// columns: the chunk of the table (FWD1_XC rows of pw double2, contiguous in memory) and each wave's 16 rows x FWD1_XC floats are fetched with
// coalesced loads into registers while the chunk before is multiplied, then handed to LDS; the k-loop reads LDS only.  The table lies in LDS
// as the B operand wants it, [x][n] with the real parts of the pw bins, then their imaginary parts, rows FWD1_EST doubles apart: the two x of
// a 32-lane group fall into opposite halves of the banks (FWD1_EST = 16 mod 32) and the read is conflict-free.  Every accumulator receives
// the k-steps of k_dft_fwd1_mfma in their order with the same operands (the float32 difference iw - mu is formed at the read, as there):
// equal bits.  The strip's rows of T, contiguous in memory, leave through LDS as whole 16-byte elements instead of 8-byte halves.
constexpr int FWD1_XC = 32, FWD1_EST = 48, FWD1_IST = 36;        // chunk; LDS row strides of the table (doubles) and of a wave's input rows (floats)
constexpr int FWD1_NLE = FWD1_XC * FWD1_MAXPW / 256, FWD1_NLI = 16 * FWD1_XC / 64;
constexpr int FWD1_LDS_E = FWD1_XC * FWD1_EST * 8, FWD1_LDS_I = 16 * FWD1_IST * 4, FWD1_LDS_O = 16 * FWD1_MAXPW * 16;
constexpr int FWD1_LDS = FWD1_LDS_E + 4 * FWD1_LDS_I > 4 * FWD1_LDS_O ? FWD1_LDS_E + 4 * FWD1_LDS_I : 4 * FWD1_LDS_O;
// NT: the column tiles, (2 pw + 15) / 16.  It is a template parameter, and every LDS read and MFMA of the k-loop unconditional (a padding column
// or a k beyond w multiplies a selected zero, as in k_dft_fwd1_mfma), so that the accumulators stay where the matrix cores leave them
// (with the occupancy bound the compiler keeps them in VGPRs; without it they were copied to AGPRs and back around every k-step).
template <int NT>
__global__ __launch_bounds__(256, 4) void k_dft_fwd1_staged(const float *__restrict__ iw, const float *__restrict__ mu, const double2 *__restrict__ Ex_all,
                                                         size_t ex_stride, double2 *__restrict__ T, int h, int w, int pw, int seg_rows, int nseg)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[FWD1_LDS];
    double *sE = (double *)s_raw;                                // [FWD1_XC][FWD1_EST]
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float *sI = (float *)(s_raw + FWD1_LDS_E) + wid * (16 * FWD1_IST);      // this wave's [16][FWD1_IST]
    const int sps = (seg_rows + 15) / 16, wgps = (sps + 3) / 4;  // strips and workgroups per segment
    const int seg = blockIdx.x / wgps, sstrip = (blockIdx.x - seg * wgps) * 4 + wid;
    const bool active = sstrip < sps;                            // a wave without a strip still stages the table and joins the barriers
    const int row0 = seg * seg_rows + sstrip * 16;
    const int row_end = (seg + 1) * seg_rows;                    // one past the segment's last row
    const int r = lane & 15, kk = lane >> 4;
    const int grow = active ? min(row0 + r, row_end - 1) : 0;    // rows past the segment repeat its last one (never stored)
    const double2 *E = Ex_all + (size_t)seg * ex_stride;
    const float m = (mu && active) ? mu[grow / h] : 0.f;
    const int ncol = 2 * pw;
    v4f64 acc[NT];
    bool colv[NT];                                               // false: padding column
#pragma unroll
    for (int t = 0; t < NT; t++) {
        acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
        colv[t] = t * 16 + r < ncol;
    }
    double2 ve[FWD1_NLE];
    float vi[FWD1_NLI];
    // every load is issued, at an index clamped into the chunk; what lies past w is dropped (table) or zeroed (input) at the hand-over
    auto fetch = [&](int xc0) {
        const int ne = min(FWD1_XC, w - xc0) * pw;               // table elements of this chunk
#pragma unroll
        for (int j = 0; j < FWD1_NLE; j++) ve[j] = E[(size_t)xc0 * pw + min((int)threadIdx.x + 256 * j, ne - 1)];
        if (active) {
#pragma unroll
            for (int j = 0; j < FWD1_NLI; j++) {
                const int e = lane + 64 * j, rr = e / FWD1_XC, x = xc0 + e % FWD1_XC;
                vi[j] = iw[(size_t)min(row0 + rr, row_end - 1) * w + min(x, w - 1)];
            }
        }
    };
    fetch(0);
    for (int xc0 = 0; xc0 < w; xc0 += FWD1_XC) {
        if (xc0) __syncthreads();                                // the chunk before has been read
        const int ne = min(FWD1_XC, w - xc0) * pw;
#pragma unroll
        for (int j = 0; j < FWD1_NLE; j++) {
            const int e = threadIdx.x + 256 * j;
            if (e < ne) {
                const int xl = e / pw, c = e - xl * pw;
                sE[xl * FWD1_EST + c] = ve[j].x;
                sE[xl * FWD1_EST + pw + c] = ve[j].y;
            }
        }
        if (active) {
#pragma unroll
            for (int j = 0; j < FWD1_NLI; j++) {
                const int e = lane + 64 * j, rr = e / FWD1_XC, xl = e % FWD1_XC;
                sI[rr * FWD1_IST + xl] = xc0 + xl < w ? vi[j] : 0.f;
            }
        }
        __syncthreads();
        if (xc0 + FWD1_XC < w) fetch(xc0 + FWD1_XC);             // in flight while this chunk is multiplied
        if (active) {
            const int nk = min(FWD1_XC, w - xc0);
            for (int xl = 0; xl < nk; xl += 4) {
                const bool in = xc0 + xl + kk < w;
                const float af = sI[r * FWD1_IST + xl + kk];
                const double a = in ? (double)__fsub_rn(af, m) : 0.0;
                double bv[NT];
#pragma unroll
                for (int t = 0; t < NT; t++) bv[t] = sE[(xl + kk) * FWD1_EST + t * 16 + r];
#pragma unroll
                for (int t = 0; t < NT; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (in && colv[t]) ? bv[t] : 0.0, acc[t], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                             // the last chunk has been read: LDS becomes the strips' rows of T
    double2 *sO = (double2 *)s_raw + wid * (16 * FWD1_MAXPW);    // this wave's [16][pw]
    if (active) {
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (!colv[t]) continue;
            const int n = t * 16 + r, c = n < pw ? n : n - pw;
#pragma unroll
            for (int q = 0; q < 4; q++) ((double *)(sO + (kk + 4 * q) * pw + c))[n < pw ? 0 : 1] = acc[t][q];
        }
    }
    __syncthreads();
    if (active) {
        const int no = min(16, row_end - row0) * pw;
        for (int e = lane; e < no; e += 64) T[(size_t)row0 * pw + e] = sO[e];
    }
}

// stage 2: patch[b, a, c] = win[a,c] * sum_y Ey[a, y] * T[b, y, c]   (complex128 spectrum value times the float32 window, as upstream's
// `patch *= win` under complex128: both parts times the window in float64)
__global__ void k_dft_fwd2(const double2 *__restrict__ T, const double2 *__restrict__ Ey_all, size_t ey_stride, const float *__restrict__ win_all,
                           int win_stride, double2 *__restrict__ patch, int h, int ph, int pw, int pstride)
{
    size_t b = blockIdx.x;
    const double2 *Ey = Ey_all + b * ey_stride;
    const float *win = win_all + b * (size_t)win_stride;
    const double2 *Tb = T + b * (size_t)h * pw;
    for (int t = threadIdx.x; t < ph * pw; t += blockDim.x) {       // one pass for patches up to 32 x 32 bins
        int a = t / pw, c = t % pw;
        double ar = 0.0, ai = 0.0;
        // one workgroup per frame: the loads of eight rows are issued together (the loop was one memory round trip per row)
        int y = 0;
        for (; y + 8 <= h; y += 8) {
            double2 e[8], v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) { e[k] = Ey[(size_t)a * h + y + k]; v[k] = Tb[(size_t)(y + k) * pw + c]; }
#pragma unroll
            for (int k = 0; k < 8; k++) cmac(ar, ai, e[k].x, e[k].y, v[k].x, v[k].y);
        }
        for (; y < h; y++) {
            const double2 e = Ey[(size_t)a * h + y], v = Tb[(size_t)y * pw + c];
            cmac(ar, ai, e.x, e.y, v.x, v.y);
        }
        const double wv = (double)win[t];
        patch[b * (size_t)pstride + t] = make_double2(ar * wv, ai * wv);
    }
}

void launch_dft_forward(const float *iw, const float *mu, const double2 *Ex, const double2 *Ey, size_t tab_stride_x, size_t tab_stride_y,
                        const float *win, double2 *tmpT, double2 *patch, int patch_stride, int B, int h, int w, int ph, int pw, hipStream_t st,
                        int win_stride, bool staged)
{
    // per-frame tables (tab_stride_x != 0): one segment per frame; a shared table: the whole batch is one segment
    const int seg_rows = tab_stride_x ? h : B * h, nseg = tab_stride_x ? B : 1;
    const int sps = (seg_rows + 15) / 16, strips = nseg * sps;
    if (staged && (dft_staged_fits(h, w, ph, pw, tab_stride_x != 0) & DFT_STAGED_FWD1)) {
        const dim3 grid(nseg * ((sps + 3) / 4));
        if (pw <= 8) hipLaunchKernelGGL(k_dft_fwd1_staged<1>, grid, dim3(256), 0, st, iw, mu, Ex, tab_stride_x, tmpT, h, w, pw, seg_rows, nseg);
        else if (pw <= 16) hipLaunchKernelGGL(k_dft_fwd1_staged<2>, grid, dim3(256), 0, st, iw, mu, Ex, tab_stride_x, tmpT, h, w, pw, seg_rows, nseg);
        else hipLaunchKernelGGL(k_dft_fwd1_staged<3>, grid, dim3(256), 0, st, iw, mu, Ex, tab_stride_x, tmpT, h, w, pw, seg_rows, nseg);
    } else
        hipLaunchKernelGGL(k_dft_fwd1_mfma, dim3((strips + 3) / 4), dim3(256), 0, st, iw, mu, Ex, tab_stride_x, tmpT, h, w, pw, seg_rows, nseg);
    hipLaunchKernelGGL(k_dft_fwd2, dim3(B), dim3(std::min(1024, ((ph * pw + 63) / 64) * 64)), 0, st, (const double2 *)tmpT, Ey, tab_stride_y, win, win_stride, patch, h,
                       ph, pw, patch_stride);
}

// stage 3: Q[b, a, x] = sum_c patch[b, a, c] * Gx[c, x]
// (geom: pair mode, rows a >= the sample's ph are never read by stage 4 and sums stop at its pw; ph / pw are the layout)
__global__ void k_dft_inv1(const double2 *__restrict__ patch, int pstride, const double2 *__restrict__ Gx_all, size_t gx_stride,
                           double2 *__restrict__ Q, int w, int ph, int pw, const CarrierGeom *__restrict__ geom)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    int a = blockIdx.y;
    size_t b = blockIdx.z;
    if (x >= w) return;
    const int pwb = geom ? max(0, min(geom[b].pw, pw)) : pw;
    if (geom && a >= max(0, min(geom[b].ph, ph))) return;
    const double2 *Gx = Gx_all + b * gx_stride;
    const double2 *pr = patch + b * (size_t)pstride + (size_t)a * pw;
    double ar = 0.0, ai = 0.0;
    for (int c = 0; c < pwb; c++) {
        const double2 p = pr[c], g = Gx[(size_t)c * w + x];
        cmac(ar, ai, p.x, p.y, g.x, g.y);
    }
    Q[(b * (size_t)ph + a) * w + x] = make_double2(ar, ai);
}

// stage 4: field[b, y, x] = sum_a Gy[y, a] * Q[b, a, x]; amp = |field| (np.abs -> float32, :997); with a reference field (cref != null: the
// deformed frames) the same thread goes on to the phase difference angle(cdef * conj(cref)) -> float32 (:1681-1689) and the amplitude
// product amp_ref * amp_def (:742), so the float64 field never travels to memory unless `field` is given (reference frame, debug planes).
// On the matrix cores: the complex product field = Gy . Q is the real float64 GEMM  [re | im] = [Gr | Gi] . [[Qr, Qi], [-Qi, Qr]]
// with K = 2 * ph: A[y][k] = Gr[y][k] for k < ph, Gi[y][k - ph] above; one double2 of Q per lane and k-step gives both B operands
// ((q.x, q.y) below ph, (-q.y, q.x) above).  A wave owns 16 rows x 64 columns of one frame (four column tiles x {re, im} accumulators), a
// workgroup four such strips; the epilogue is that of k_dft_inv2 (re and im of an element sit in the same lane and register index).
__global__ __launch_bounds__(256) void k_dft_inv2_mfma(const double2 *__restrict__ Q, const double2 *__restrict__ Gy_all, size_t gy_stride,
                                                       double2 *__restrict__ field, float *__restrict__ amp, const double2 *__restrict__ cref_all,
                                                       const float *__restrict__ amp_ref_all, size_t ref_stride, float *__restrict__ prod,
                                                       float *__restrict__ wrapped, int h, int w, int ph, const CarrierGeom *__restrict__ geom)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 64, y0 = (blockIdx.y * 4 + wid) * 16;
    const size_t b = blockIdx.z;
    if (y0 >= h) return;
    const int r = lane & 15, kk = lane >> 4;
    const double *G = (const double *)(Gy_all + b * gy_stride);
    const double2 *Qb = Q + b * (size_t)ph * w;
    const int ya = min(y0 + r, h - 1);
    v4f64 cre[4], cim[4];
    const int phb = geom ? max(0, min(geom[b].ph, ph)) : ph;     // the sample's own extent: K and the re / im split as a launch of that size
    cgemm16x64_mfma(G, ph, phb, Qb, w, w, ya, x0, lane, cre, cim);
    const double2 *cref = cref_all ? cref_all + b * ref_stride : nullptr;
    const float *amp_ref = amp_ref_all ? amp_ref_all + b * ref_stride : nullptr;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int x = x0 + 16 * t + r;
        if (x >= w) continue;
#pragma unroll
        for (int qd = 0; qd < 4; qd++) {
            const int y = y0 + kk + 4 * qd;
            if (y >= h) continue;
            const double ar = cre[t][qd], ai = cim[t][qd];
            const size_t p = (size_t)y * w + x, i = b * (size_t)h * w + p;
            if (field) field[i] = make_double2(ar, ai);
            const float am = (float)sqrt(fma(ar, ar, ai * ai));
            amp[i] = am;
            if (cref) {
                const double2 c = cref[p];
                const double rr = ar * c.x + ai * c.y;
                const double ri = ai * c.x - ar * c.y;
                wrapped[i] = (float)atan2(ri, rr);
                prod[i] = __fmul_rn(amp_ref[p], am);
            }
        }
    }
}

// the epilogue of stage 4 for one 16 x 16 tile: the lane's column x and its four rows y + 4 qd (re and im of an element sit in the same lane and
// register index), for k_dft_inv2_staged.  The expressions are those of k_dft_inv2_mfma's epilogue, which stays as it was compiled: the bits of
// amp, wrapped and prod hang on them.
// cv / av: cref and amp_ref at the tile's four pixels (fetched at clamped positions by the caller; read only where cref is given).
__device__ __forceinline__ void inv2_finish_tile(const v4f64 &cre, const v4f64 &cim, int x, int y, size_t b, int h, int w, double2 *__restrict__ field,
                                                 float *__restrict__ amp, bool cref, const double2 (&cv)[4], const float (&av)[4],
                                                 float *__restrict__ prod, float *__restrict__ wrapped)
{
    if (x >= w) return;
#pragma unroll
    for (int qd = 0; qd < 4; qd++, y += 4) {
        if (y >= h) continue;
        const double ar = cre[qd], ai = cim[qd];
        const size_t p = (size_t)y * w + x, i = b * (size_t)h * w + p;
        if (field) field[i] = make_double2(ar, ai);
        const float am = (float)sqrt(fma(ar, ar, ai * ai));
        amp[i] = am;
        if (cref) {
            const double2 c = cv[qd];
            const double rr = ar * c.x + ai * c.y;
            const double ri = ai * c.x - ar * c.y;
            wrapped[i] = (float)atan2(ri, rr);
            prod[i] = __fmul_rn(av[qd], am);
        }
    }
}

// stage 4 with its operands staged in LDS (Tiers::dft_staged, patches dft_staged_fits takes): the same grid, the same tile per wave and the
// same k-steps as k_dft_inv2_mfma, fed differently.  The workgroup loads its 64 columns of Q once for its four waves (ph x 64 double2, coalesced
// 16-byte loads, all in flight together), each wave its 16 rows of Gy (contiguous in memory); the k-loop reads LDS only (cgemm16_lds_mfma).
// A wave walks its four column tiles in passes of INV2_NT and finishes each pass before the next starts, so 2 INV2_NT accumulators instead of
// eight are live across the epilogue; tiles wholly beyond w are skipped (at w = 224 an eighth of the parent's MFMAs).  An accumulator still
// receives the k-steps of the parent in their order with the same operands: equal bits.  LDS: 2 KB per row of the patch + 4 KB.  The
// reference field and amplitude of a pass's pixels are fetched before its k-loop, so that they arrive while the matrix cores work.
constexpr int INV2_NT = 2;
__global__ __launch_bounds__(256, 3) void k_dft_inv2_staged(const double2 *__restrict__ Q, const double2 *__restrict__ Gy_all, size_t gy_stride,
                                                         double2 *__restrict__ field, float *__restrict__ amp, const double2 *__restrict__ cref_all,
                                                         const float *__restrict__ amp_ref_all, size_t ref_stride, float *__restrict__ prod,
                                                         float *__restrict__ wrapped, int h, int w, int ph, const CarrierGeom *__restrict__ geom)
{
    extern __shared__ double2 s_inv2[];                          // Q columns [ph][64], the four waves' Gy rows [16][ph] each, 256 spare elements
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 64, y0 = (blockIdx.y * 4 + wid) * 16;
    const size_t b = blockIdx.z;
    const int r = lane & 15, kk = lane >> 4;
    const double2 *Qb = Q + b * (size_t)ph * w;
    const int phb = geom ? max(0, min(geom[b].ph, ph)) : ph;     // the sample's own extent: K and the re / im split as a launch of that size
    double2 *sQ = s_inv2, *sG = s_inv2 + ph * 64 + wid * 16 * ph;
    constexpr int NLD = (INV2_MAXPH * 64 + 255) / 256;
    // Every load is issued, at an index clamped into what is staged, and every store too (what is not staged goes to a spare element per
    // thread behind the images): no branch stands between the loads, one round trip for all of them.
    const int spare = ph * 128 + threadIdx.x;
    if (phb > 0) {  // rows 0..phb-1 of Q (the rows beyond are never read: pair mode leaves them unwritten), columns clamped to w - 1 as the parent's loads
        double2 v[NLD];
        const int c = min(x0 + lane, w - 1);
#pragma unroll
        for (int j = 0; j < NLD; j++) v[j] = Qb[(size_t)min(wid + 4 * j, phb - 1) * w + c];
#pragma unroll
        for (int j = 0; j < NLD; j++) sQ[wid + 4 * j < phb ? (wid + 4 * j) * 64 + lane : spare] = v[j];
    }
    if (y0 < h) {
        const double2 *Gs = Gy_all + b * gy_stride + (size_t)y0 * ph;
        const int n = min(16, h - y0) * ph;
        double2 v[NLD];
#pragma unroll
        for (int j = 0; j < NLD; j++) v[j] = Gs[min(lane + 64 * j, n - 1)];
#pragma unroll
        for (int j = 0; j < NLD; j++) (lane + 64 * j < n ? sG + lane + 64 * j : sQ + spare)[0] = v[j];
    }
    __syncthreads();
    if (y0 >= h) return;
    const int ra = min(r, h - 1 - y0);                           // rows past the frame repeat its last one (never stored)
    const double2 *cref = cref_all ? cref_all + b * ref_stride : nullptr;
    const float *amp_ref = amp_ref_all ? amp_ref_all + b * ref_stride : nullptr;
    for (int t0 = 0; t0 < 4 && x0 + 16 * t0 < w; t0 += INV2_NT) {
        v4f64 cre[INV2_NT], cim[INV2_NT];
        double2 cv[INV2_NT][4];
        float av[INV2_NT][4];
        if (cref) {
#pragma unroll
            for (int t = 0; t < INV2_NT; t++)
#pragma unroll
                for (int qd = 0; qd < 4; qd++) {
                    const size_t p = (size_t)min(y0 + kk + 4 * qd, h - 1) * w + min(x0 + 16 * (t0 + t) + r, w - 1);
                    cv[t][qd] = cref[p];
                    av[t][qd] = amp_ref[p];
                }
        }
        cgemm16_lds_mfma<INV2_NT>((const double *)sG, ph, phb, sQ, ra, t0, lane, cre, cim);
#pragma unroll
        for (int t = 0; t < INV2_NT; t++)
            inv2_finish_tile(cre[t], cim[t], x0 + 16 * (t0 + t) + r, y0 + kk, b, h, w, field, amp, cref != nullptr, cv[t], av[t], prod, wrapped);
    }
}

void launch_dft_inverse(const double2 *patch, int patch_stride, const double2 *Gx, const double2 *Gy, size_t tab_stride_x, size_t tab_stride_y,
                        double2 *tmpQ, double2 *field, float *amp, const double2 *cref, const float *amp_ref, size_t ref_stride, float *prod,
                        float *wrapped, int B, int h, int w, int ph, int pw, hipStream_t st, const CarrierGeom *geom, bool staged)
{
    hipLaunchKernelGGL(k_dft_inv1, dim3((w + 255) / 256, ph, B), dim3(256), 0, st, patch, patch_stride, Gx, tab_stride_x, tmpQ, w, ph, pw, geom);
    const dim3 grid((w + 63) / 64, (h + 63) / 64, B);
    if (staged && (dft_staged_fits(h, w, ph, pw, tab_stride_x != 0) & DFT_STAGED_INV2))
        hipLaunchKernelGGL(k_dft_inv2_staged, grid, dim3(256), (size_t)ph * 2048 + 4096, st, (const double2 *)tmpQ, Gy, tab_stride_y, field, amp, cref, amp_ref,
                           ref_stride, prod, wrapped, h, w, ph, geom);
    else
        hipLaunchKernelGGL(k_dft_inv2_mfma, grid, dim3(256), 0, st, (const double2 *)tmpQ, Gy, tab_stride_y, field, amp, cref, amp_ref, ref_stride, prod,
                           wrapped, h, w, ph, geom);
}

// ---- full spectrum magnitude (reference-frame carrier search, shape_ftp.py:867-872), float64 as np.abs(fft2(float64)) ----
// The frame is real, so F(-f) = conj F(f): only the columns fx = 0 .. Wf/2 are computed (stage 1 = k_dft_fwd1_mfma with the half table
// as its "patch", stage 2 below) and every magnitude is written to its own and to its mirror position of the fftshift-ed plane.
// Stage 2: mag[fy][fx] = | sum_y Eyf[fy][y] * T[y][fx] |, the complex product as the real float64 GEMM of k_dft_inv2_mfma (K = 2h); a wave
// owns 16 frequency rows x 64 columns.
__global__ __launch_bounds__(256) void k_full2_mfma(const double2 *__restrict__ T, const double2 *__restrict__ Eyf, double *__restrict__ mag_all,
                                                    int h, int Hf, int Wf, int Wh)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 64, y0 = (blockIdx.y * 4 + wid) * 16;
    const size_t b = blockIdx.z;
    if (y0 >= Hf) return;
    const int r = lane & 15, kk = lane >> 4;
    const double *G = (const double *)Eyf;
    const double2 *Tb = T + b * (size_t)h * Wh;
    const int ya = min(y0 + r, Hf - 1);
    v4f64 cre[4], cim[4];
    cgemm16x64_mfma(G, h, h, Tb, Wh, Wh, ya, x0, lane, cre, cim);
    double *mag = mag_all + b * (size_t)Hf * Wf;
    const int cy = Hf / 2, cx = Wf / 2;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int fx = x0 + 16 * t + r;
        if (fx >= Wh) continue;
#pragma unroll
        for (int qd = 0; qd < 4; qd++) {
            const int fy = y0 + kk + 4 * qd;
            if (fy >= Hf) continue;
            const double ar = cre[t][qd], ai = cim[t][qd];
            const double m = sqrt(fma(ar, ar, ai * ai));
            mag[(size_t)((fy + cy) % Hf) * Wf + (fx + cx) % Wf] = m;
            const int mx = (Wf - fx) % Wf;                       // mirror column: outside the computed half unless fx is 0 or Wf/2
            if (mx >= Wh) mag[(size_t)(((Hf - fy) % Hf + cy) % Hf) * Wf + (mx + cx) % Wf] = m;
        }
    }
}

// stage 1 alone with one table for the batch: T[b*h + y][c] = sum_x (iw[b][y][x] - mu[b]) * Ex[x][c], c = 0..nc-1 (mu may be null)
void launch_dft_rows(const float *iw, const float *mu, const double2 *Ex, double2 *T, int B, int h, int w, int nc, hipStream_t st)
{
    const int rows = B * h;
    hipLaunchKernelGGL(k_dft_fwd1_mfma, dim3(((rows + 15) / 16 + 3) / 4), dim3(256), 0, st, iw, mu, Ex, (size_t)0, T, h, w, nc, rows, 1);
}

// Ex_half: [w][Wh] (Wh = Wf/2 + 1), Ey_full: [Hf][h]; tmp: [B*h][Wh] double2
void launch_dft_full_mag(const float *iw, const float *mu, const double2 *Ex_half, const double2 *Ey_full, double2 *tmp,
                         double *mag, int B, int h, int w, int Hf, int Wf, hipStream_t st)
{
    const int Wh = Wf / 2 + 1;
    launch_dft_rows(iw, mu, Ex_half, tmp, B, h, w, Wh, st);
    hipLaunchKernelGGL(k_full2_mfma, dim3((Wh + 63) / 64, (Hf + 63) / 64, B), dim3(256), 0, st, (const double2 *)tmp, Ey_full, mag, h, Hf, Wf, Wh);
}

// top-N magnitudes outside the DC box (find_top_peaks, shape_ftp.py:420-441), descending: out[b][3*i] = x, y, value.  One workgroup
// per frame.  Magnitudes are non-negative doubles: their bit patterns order like the values.  ONE pass over the plane: every thread keeps
// the TP_L largest of its strided elements (value bits, index) in registers; the N largest of the frame are then among the 1024 * TP_L
// survivors unless one thread held more than TP_L of them -- detected (the best element that thread discarded then comes before the N-th
// result in the order below; a plane with fewer than N positive values included, where the N-th result is a zero) and handled by the exact
// N-pass fallback.  Equal values: smaller linear index first.
constexpr int TP_L = 4;
__device__ inline bool tp_before(unsigned long long va, unsigned int ia, unsigned long long vb, unsigned int ib) { return va > vb || (va == vb && ia < ib); }

__global__ __launch_bounds__(1024) void k_top_peaks(const double *__restrict__ mag_all, int Hf, int Wf, int dc, int npeaks, double *__restrict__ out_all)
{
    __shared__ unsigned long long scratch[16];
    __shared__ unsigned int chosen[64];
    __shared__ unsigned long long s_val[1024 * TP_L];
    __shared__ unsigned int s_idx[1024 * TP_L];
    __shared__ int s_overflow;
    const size_t n = (size_t)Hf * Wf;
    const double *mag = mag_all + blockIdx.x * n;
    double *out = out_all + blockIdx.x * (size_t)(3 * 64);
    const int tid = threadIdx.x;
    int cy = Hf / 2, cx = Wf / 2;
    int y0 = max(0, cy - dc), y1 = min(Hf, cy + dc), x0 = max(0, cx - dc), x1 = min(Wf, cx + dc);
    if (npeaks > 64) npeaks = 64;
    // ---- per-thread top TP_L (sorted, best first); `dropped` = the best element this thread had to discard
    unsigned long long tv[TP_L], dropped_v = 0;
    unsigned int ti[TP_L], dropped_i = 0xffffffffu;
    bool dropped = false;
#pragma unroll
    for (int k = 0; k < TP_L; k++) { tv[k] = 0ull; ti[k] = 0xffffffffu; }
    for (size_t i = tid; i < n; i += 1024) {
        const int y = (int)(i / Wf), x = (int)(i % Wf);
        double v = mag[i];
        if (y >= y0 && y < y1 && x >= x0 && x < x1) v = 0.0;
        unsigned long long cv = (unsigned long long)__double_as_longlong(v);
        unsigned int ci = (unsigned int)i;
        if (!tp_before(cv, ci, tv[TP_L - 1], ti[TP_L - 1])) {       // not better than the worst kept: discard
            if (!dropped || tp_before(cv, ci, dropped_v, dropped_i)) { dropped_v = cv; dropped_i = ci; }
            dropped = true;
            continue;
        }
        if (ti[TP_L - 1] != 0xffffffffu) {
            if (!dropped || tp_before(tv[TP_L - 1], ti[TP_L - 1], dropped_v, dropped_i)) { dropped_v = tv[TP_L - 1]; dropped_i = ti[TP_L - 1]; }
            dropped = true;
        }
#pragma unroll
        for (int k = 0; k < TP_L; k++) {                            // sorted insertion
            if (tp_before(cv, ci, tv[k], ti[k])) { const unsigned long long xv = tv[k]; const unsigned int xi = ti[k]; tv[k] = cv; ti[k] = ci; cv = xv; ci = xi; }
        }
    }
#pragma unroll
    for (int k = 0; k < TP_L; k++) { s_val[tid * TP_L + k] = tv[k]; s_idx[tid * TP_L + k] = ti[k]; }
    if (tid == 0) s_overflow = 0;
    __syncthreads();
    // ---- N rounds of block-wide arg-max over the survivors
    unsigned long long last_v = 0;
    unsigned int last_i = 0xffffffffu;
    for (int k = 0; k < npeaks; k++) {
        unsigned long long bv = 0;
        unsigned int bi = 0xffffffffu;
        for (int j = tid; j < 1024 * TP_L; j += 1024) {
            const unsigned long long v = s_val[j];
            const unsigned int ix = s_idx[j];
            if (ix != 0xffffffffu && tp_before(v, ix, bv, bi)) { bv = v; bi = ix; }
        }
        const unsigned long long mv = block_max_u64(bv, scratch);
        __syncthreads();
        const unsigned long long mi = block_min_u64(bv == mv && bi != 0xffffffffu ? (unsigned long long)bi : ~0ull, scratch);
        if (tid == 0) {
            chosen[k] = (unsigned int)mi;
            out[3 * k] = (double)((unsigned int)mi % Wf);
            out[3 * k + 1] = (double)((unsigned int)mi / Wf);
            out[3 * k + 2] = __longlong_as_double((long long)mv);
        }
        for (int j = tid; j < 1024 * TP_L; j += 1024)
            if (s_idx[j] == (unsigned int)mi) s_idx[j] = 0xffffffffu;
        last_v = mv; last_i = (unsigned int)mi;
        __syncthreads();
    }
    // a discarded element that would have made the list: redo exactly (never seen on spectra: the peaks are few and far apart).  The test is
    // the order itself, so an all-zero plane (every discarded zero lies behind the N-th index) stays on the one pass
    if (dropped && tp_before(dropped_v, dropped_i, last_v, last_i)) s_overflow = 1;
    __syncthreads();
    if (!s_overflow) return;
    for (int k = 0; k < npeaks; k++) {
        unsigned long long best = 0;
        for (size_t i = tid; i < n; i += 1024) {
            int y = (int)(i / Wf), x = (int)(i % Wf);
            double v = mag[i];
            if (y >= y0 && y < y1 && x >= x0 && x < x1) v = 0.0;
            bool skip = false;
            for (int j = 0; j < k; j++) skip |= (chosen[j] == (unsigned int)i);
            if (skip) continue;
            const unsigned long long key = (unsigned long long)__double_as_longlong(v);
            if (key > best) best = key;
        }
        best = block_max_u64(best, scratch);
        __syncthreads();
        unsigned long long idx = ~0ull;
        for (size_t i = tid; i < n; i += 1024) {
            int y = (int)(i / Wf), x = (int)(i % Wf);
            double v = mag[i];
            if (y >= y0 && y < y1 && x >= x0 && x < x1) v = 0.0;
            bool skip = false;
            for (int j = 0; j < k; j++) skip |= (chosen[j] == (unsigned int)i);
            if (!skip && (unsigned long long)__double_as_longlong(v) == best && i < idx) idx = i;
        }
        idx = block_min_u64(idx, scratch);
        if (tid == 0) {
            chosen[k] = (unsigned int)idx;
            out[3 * k] = (double)(idx % Wf);
            out[3 * k + 1] = (double)(idx / Wf);
            out[3 * k + 2] = __longlong_as_double((long long)best);
        }
        __syncthreads();
    }
}

void launch_top_peaks(const double *mag, int B, int Hf, int Wf, int dc, int npeaks, double *out_xyv, hipStream_t st)
{
    hipLaunchKernelGGL(k_top_peaks, dim3(B), dim3(1024), 0, st, mag, Hf, Wf, dc, npeaks, out_xyv);
}

}  // namespace vf
