// td7_pink.hip -- coloured (power-law) exploration noise, one sequence per env.
//
//   td7f_pink_advance : the per-episode noise of Agent/TD7_multi_agent_Pink_noise.py
//                       :203-228 (one power-law sequence per episode, peak
//                       normalised, times the exploration noise at the start of
//                       the episode; column t is added to the action of step t)
//                       for n envs with asynchronous episodes: every env has its
//                       own sequence of its own motion length, regenerated in the
//                       launch after the step that ended its episode.
//
// One workgroup per env; a workgroup whose env is not flagged `done` at most
// counts its step and leaves.  A flagged env follows pink.powerlaw_psd_gaussian
// (Timmer & Koenig 1995) on its row of the table seq [n][Lmax][A]:
//
//   spectrum   sr_k = z0 scale_k, si_k = z1 scale_k, (z0, z1) the Box-Muller
//              pair of Philox block j = ((r - seg[p]) A + c) nf_max + k of call
//              epi[r] of policy p's stream -- segment-local, so what a policy
//              draws depends neither on its neighbours nor on where its segment
//              starts -- or the given spectra (tests).
//   masking    si_0 = 0, sr_0 *= sqrt 2; for even n the same at k = n / 2.
//   inverse    x[t] = norm (sr_0 + 2 sum_k (sr_k cos(2 pi k t / n) - si_k
//              sin(2 pi k t / n))), the Nyquist term without the 2: a direct
//              real DFT in fp32.  The motion lengths (232..347) are neither
//              powers of two nor shared between rows, so no FFT library; the
//              longest row is 7 x 347 x 174 multiply-adds.  The twiddles are an
//              LDS table of sincospi(2 m / n), m < n, indexed by k t mod n, which
//              is stepped (idx += t, one conditional subtraction): no division.
//              Thread t owns time step t for all A columns: the spectrum reads
//              are wave-uniform (LDS broadcast), the factors 1 / 2 of the sum
//              are folded into the LDS spectrum when it is written.
//   peak       max |x| over the row's [n][A] block (block reduction);
//              seq[r][t][c] = x * (sigma_p / peak), sigma_p as it stands now:
//              frozen for the episode, as the reference does.  peak == 0: gain 0.
//
// Every store to t, epi and seq is an ordinary per-thread vector store.
#include "td7_fused.h"

#include <algorithm>

namespace td7f {

constexpr int PNT = 384;  // 6 waves: one pass over the longest motion (347 steps)
constexpr int PAP = 8;    // columns of the LDS spectrum (A <= 8, zero padded)
constexpr int PINK_LDS_MAX = 64 * 1024;

struct PinkArgs {
    const uint8_t *stepped, *done;
    int *t, *epi;
    float *seq;
    const int *len_cls, *cls_len;
    const float *cls_norm, *cls_scale;
    const td7f_noise_row *nzt;
    const int *seg;
    const float *spectrum;
    float *spec_out, *peak_out;
    int npol, A, Lmax, nf_max, ncls;
    int off_tw, off_x, off_red;
};

__global__ __launch_bounds__(PNT) void pink_advance_kernel(PinkArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (!ldg(a.done + r)) {
        if (tid == 0 && ldg(a.stepped + r)) stg(a.t + r, ldg(a.t + r) + 1);
        return;
    }
    // the policy of row r: seg[p] <= r < seg[p + 1] (empty segments skipped)
    int p = 0;
    while (p + 1 < a.npol && ldg(a.seg + p + 1) <= r) ++p;
    const int seg0 = ldg(a.seg + p);
    const td7f_noise_row *row = a.nzt + p;
    const uint64_t seed = ldg(&row->seed);
    const uint32_t tag = ldg(&row->tag);
    const int call = ldg(a.epi + r) + 1;  // the episode that starts now
    const int cls = min(max(ldg(a.len_cls + r), 0), a.ncls - 1);
    const int n = min(max(ldg(a.cls_len + cls), 2), a.Lmax), nf = n / 2 + 1;
    const float norm = ldg(a.cls_norm + cls);
    const float *scale = a.cls_scale + (size_t)cls * a.nf_max;
    const int A = a.A;

    float2 *spec = (float2 *)lds;             // [nf][PAP]: (w sr, w si), w = 2 (1 at k = 0 and Nyquist)
    float2 *tw = (float2 *)(lds + a.off_tw);  // [n]: (cos, sin)(2 pi m / n)
    float *xs = (float *)(lds + a.off_x);     // [n][A]
    float *red = (float *)(lds + a.off_red);  // [PNT / 64]

    for (int i = tid; i < nf * PAP; i += PNT) {
        const int k = i / PAP, c = i - k * PAP;
        float2 v = {0.f, 0.f};
        if (c < A) {
            const size_t e = ((size_t)r * A + c) * a.nf_max + k;
            float sr, si;
            if (a.spectrum) {
                sr = ldg(a.spectrum + 2 * e);
                si = ldg(a.spectrum + 2 * e + 1);
            } else {
                const uint32_t j = (uint32_t)((r - seg0) * A + c) * (uint32_t)a.nf_max + (uint32_t)k;
                uint32_t b[4];
                philox_block(seed, tag, (uint64_t)(uint32_t)call, j, b);
                float z0, z1;
                box_muller(b, z0, z1);
                const float sc = ldg(scale + k);
                sr = z0 * sc;
                si = z1 * sc;
            }
            if (a.spec_out) {
                stg(a.spec_out + 2 * e, sr);
                stg(a.spec_out + 2 * e + 1, si);
            }
            float w = 2.f;
            if (k == 0 || 2 * k == n) {
                sr *= 1.41421356237309505f;
                si = 0.f;
                w = 1.f;
            }
            v = float2{w * sr, w * si};
        }
        spec[i] = v;
    }
    for (int m = tid; m < n; m += PNT) {
        // the angle in (-pi, pi]: the quotient's rounding is relative to a value <= 1
        const int mm = 2 * m > n ? m - n : m;
        float s, c;
        sincospif(2.0f * (float)mm / (float)n, &s, &c);
        tw[m] = float2{c, s};
    }
    __syncthreads();

    float peak = 0.f;
    for (int t = tid; t < n; t += PNT) {
        float acc[PAP];
#pragma unroll
        for (int c = 0; c < PAP; ++c) acc[c] = 0.f;
        int idx = 0;  // k t mod n
        for (int k = 0; k < nf; ++k) {
            const float2 w = tw[idx];
            const floatx4 *sp = (const floatx4 *)(spec + k * PAP);
#pragma unroll
            for (int q = 0; q < PAP / 2; ++q) {
                const floatx4 v = sp[q];  // two columns: (sr, si, sr, si)
                acc[2 * q] = fmaf(-v[1], w.y, fmaf(v[0], w.x, acc[2 * q]));
                acc[2 * q + 1] = fmaf(-v[3], w.y, fmaf(v[2], w.x, acc[2 * q + 1]));
            }
            idx += t;
            if (idx >= n) idx -= n;
        }
#pragma unroll
        for (int c = 0; c < PAP; ++c)
            if (c < A) {
                const float x = norm * acc[c];
                xs[t * A + c] = x;
                peak = fmaxf(peak, fabsf(x));
            }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) peak = fmaxf(peak, __shfl_xor(peak, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = peak;
    __syncthreads();
    peak = red[0];
#pragma unroll
    for (int w = 1; w < PNT / 64; ++w) peak = fmaxf(peak, red[w]);

    const float sg = ldg(ldg(&row->sigma));
    const float gain = peak > 0.f ? sg / peak : 0.f;
    float *out = a.seq + (size_t)r * a.Lmax * A;
    for (int i = tid; i < n * A; i += PNT) stg(out + i, xs[i] * gain);
    if (tid == 0) {
        if (a.peak_out) stg(a.peak_out + r, peak);
        stg(a.t + r, 0);
        stg(a.epi + r, call);
    }
}

}  // namespace td7f

using namespace td7f;

extern "C" int td7f_pink_advance(int32_t npol, const int32_t *seg, int32_t n, int32_t A, int32_t Lmax, int32_t ncls,
                                 const int32_t *cls_len, const uint8_t *stepped_dev, const uint8_t *done_dev,
                                 int32_t *t_dev, int32_t *epi_dev, float *seq_dev, const int32_t *len_cls_dev,
                                 const int32_t *cls_len_dev, const float *cls_norm_dev, const float *cls_scale_dev,
                                 const td7f_noise_row *noise, const void *noise_dev, const int32_t *seg_dev,
                                 const float *spectrum_dev, float *spec_out_dev, float *peak_out_dev, void *stream) {
    if (npol <= 0 || !seg || n <= 0 || A <= 0 || A > PAP || Lmax < 2 || ncls <= 0 || !cls_len || !stepped_dev ||
        !done_dev || !t_dev || !epi_dev || !seq_dev || !len_cls_dev || !cls_len_dev || !cls_norm_dev ||
        !cls_scale_dev || !noise || !noise_dev || !seg_dev)
        return EXO_EINVAL;
    if (seg[0] != 0 || seg[npol] != n) return EXO_EINVAL;
    const int nf_max = Lmax / 2 + 1;
    for (int p = 0; p < npol; ++p) {
        if (seg[p + 1] < seg[p]) return EXO_EINVAL;
        if (seg[p + 1] > seg[p] && !noise[p].sigma) return EXO_EINVAL;
        // the Philox block index of a policy's last element is 32 bits
        if ((long long)(seg[p + 1] - seg[p]) * A * nf_max > (1LL << 32)) return EXO_ERANGE;
    }
    for (int c = 0; c < ncls; ++c)
        if (cls_len[c] < 2 || cls_len[c] > Lmax) return EXO_EINVAL;
    PinkArgs a{};
    a.stepped = stepped_dev;
    a.done = done_dev;
    a.t = t_dev;
    a.epi = epi_dev;
    a.seq = seq_dev;
    a.len_cls = len_cls_dev;
    a.cls_len = cls_len_dev;
    a.cls_norm = cls_norm_dev;
    a.cls_scale = cls_scale_dev;
    a.nzt = (const td7f_noise_row *)noise_dev;
    a.seg = seg_dev;
    a.spectrum = spectrum_dev;
    a.spec_out = spec_out_dev;
    a.peak_out = peak_out_dev;
    a.npol = npol;
    a.A = A;
    a.Lmax = Lmax;
    a.nf_max = nf_max;
    a.ncls = ncls;
    a.off_tw = nf_max * PAP * 8;
    a.off_x = a.off_tw + round_up(Lmax * 8, 16);
    a.off_red = a.off_x + round_up(Lmax * A * 4, 16);
    const int lds = a.off_red + (PNT / 64) * 4;
    if (lds > PINK_LDS_MAX) return EXO_EINVAL;
    if (td7f_probe_mode) return EXO_OK;
    hipLaunchKernelGGL(pink_advance_kernel, dim3((unsigned)n), dim3(PNT), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? EXO_OK : EXO_EDEVICE;
}
