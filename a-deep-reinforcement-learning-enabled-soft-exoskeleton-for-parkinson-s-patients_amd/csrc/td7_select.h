// td7_select.h -- the networks of Agent.select_action on one workgroup's rows
// and their LDS plan, shared by select_kernel (td7_fused.hip) and the
// multi-policy kernels (td7_fused_multi.hip): one body, so the launches agree
// bit for bit by construction.
#pragma once
#include <algorithm>

#include "td7_fused.h"

namespace td7f {

// What every select launch knows about its rows: shapes, the observation and
// action tensors (n rows), the launch-wide noise state and the LDS images.  F
// (the fp32 norm input) overlays H1 | H2, dead whenever F is written, when it
// fits there (select_plan).  The images' total size, lds_bytes, stands beside
// the plan in the argument structs, not in it: as the plan's last member it
// would be followed by tail padding, and select_kernel's first scalar load of
// the images then no longer takes in tile0 (one more scalar-load wait in every
// 16-row workgroup: profiles/select_shared).
struct SelectPlan {
    int act_enc, act_actor;
    const float *obs;
    int n, S, A, Z, Ha;
    float *out;
    Noise nz;
    R16 X, H1, H2, CAT;
    R32 F, TW, FT;
};

__device__ __forceinline__ R16 rows_of(R16 r, int t) { return R16{r.off + t * TR * r.ld * 2, r.ld}; }
__device__ __forceinline__ R32 rows_of(R32 r, int t) { return R32{r.off + t * TR * r.ld * 4, r.ld}; }

// select_action's networks (Agent/TD7_multi_agent.py:72-77, :93-97) on the
// rows [row0, row0 + 16 RT) below `nrows` (rows at or past it are neither read
// nor written): leaves tanh(l3(...)) in the fp32 region a.FT.  Every thread of
// the workgroup calls it; it ends with a barrier.  The plan comes by value: by
// reference the 32-row and ZM 2 kernels allocate more registers (same source
// otherwise; profiles/select_shared).
// layer(i): layer i of zs1..zs3, l0..l3 as a Lin (or a reference to one), asked
// for just before the group that needs it -- (zs1, l3), (zs2, zs3, l0),
// (l1, l2) -- so a caller that loads them from memory never holds all seven.
// ZM (td7f_select_part): 0 the whole pass; 1 the fixed encoder's zs only, its
// normalised image stored to zimg ([nrows][Z], operand type; no actor: the
// caller returns); 2 the actor from that image (the zs layers skipped).  The
// image is the operand-type values ZM 0 leaves in CAT, so 1 + 2 == 0 bit for
// bit (same row tiles).
template <int P, int TH, int RT, int ZM, typename Layers>
__device__ __forceinline__ void select_rows(char *lds, const SelectPlan a, int lds_bytes, int row0, int nrows,
                                            void *zimg, const Layers &layer) {
    constexpr int rows = RT * TR;
    int si = 0;
    FSTAMP(si);
    const auto &first = layer(ZM == 2 ? 3 : 0), &l3 = layer(6);
    RowStage so[RT];
    ThinStage<THIN_NC> tw;
    using E = typename Ty<P>::E;
    static_assert(RT * TR * (int)sizeof(E) <= 64, "ZM 2 staging: 16 rows x 512 words at most");
#pragma unroll
    for (int t = 0; t < RT; ++t) row_issue(so[t], a.obs, a.S, a.S, row0 + t * TR, nrows);
    if constexpr (ZM != 1) thin_issue(tw, l3.w, l3.ldw, 0, false, a.A, l3.K);
    // ZM 2: this workgroup's zs image rows in 4-byte words (Z * EB % 4 == 0,
    // at most 16 rows x 512 words per 512 threads: checked on the host),
    // loaded with the observations
    const int zw = a.Z * (int)sizeof(E) / 4;
    constexpr int ZPT = ZM == 2 ? (16 * 512 + NTH - 1) / NTH : 1;
    uint32_t zv[ZPT];
    if constexpr (ZM == 2) {
        const uint32_t *zi = (const uint32_t *)zimg;
#pragma unroll
        for (int u = 0; u < ZPT; ++u) {
            const int k = threadIdx.x + u * NTH, r = k / zw, c = k - r * zw;
            zv[u] = (r < rows && row0 + r < nrows) ? zi[(long)(row0 + r) * zw + c] : 0u;
        }
    }
    Ring<TH> R;
    ring_fill<TH>(R, GDesc{first.wf, first.ksf, 0});
    zero_lds(lds, lds_bytes);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < RT; ++t) row_put16<P>(lds, so[t], rows_of(a.X, t), 0, a.S, row0 + t * TR, nrows);
    if constexpr (ZM != 1) thin_put<P>(lds, tw, a.TW, a.A, l3.K);
    if constexpr (ZM == 2) {
#pragma unroll
        for (int u = 0; u < ZPT; ++u) {
            const int k = threadIdx.x + u * NTH, r = k / zw, c = k - r * zw;
            if (r < rows) *(uint32_t *)(pe<P>(lds, a.CAT, r, a.Ha) + c * (4 / (int)sizeof(E))) = zv[u];
        }
    }
    __syncthreads();
    const auto &l0 = layer(3);
    if constexpr (ZM != 2) {
        // zs = fixed_encoder.zs(obs) (:93-97) -> CAT[:, Ha:Ha+Z]
        const auto &zs2 = layer(1), &zs3 = layer(2);
        layer_fwd<P, RT, TH>(lds, R, a.X, first, &zs2, a.act_enc, a.H1, 0, NO32, nullptr, 0, row0, nrows, si);
        layer_fwd<P, RT, TH>(lds, R, a.H1, zs2, &zs3, a.act_enc, a.H2, 0, NO32, nullptr, 0, row0, nrows, si);
        layer_fwd<P, RT, TH>(lds, R, a.H2, zs3, ZM == 1 ? (const Lin *)nullptr : &l0, ACT_NONE, NO16, 0, a.F, nullptr,
                             0, row0, nrows, si);
        norm_fwd<P>(lds, a.F, a.Z, rows, 1e-8f, a.CAT, a.Ha, NO16, 0, NO32, nullptr, 0, nullptr, nullptr, row0, nrows);
        __syncthreads();
    }
    if constexpr (ZM == 1) {
        uint32_t *zo = (uint32_t *)zimg;
        for (int k = threadIdx.x; k < rows * zw; k += NTH) {
            const int r = k / zw, c = k - r * zw;
            if (row0 + r < nrows)
                zo[(long)(row0 + r) * zw + c] = *(const uint32_t *)(pe<P>(lds, a.CAT, r, a.Ha) + c * (4 / (int)sizeof(E)));
        }
        return;
    }
    // actor (:72-77): AvgL1Norm(l0(s)) | zs -> l1 -> l2 -> tanh(l3)
    const auto &l1 = layer(4), &l2 = layer(5);
    layer_fwd<P, RT, TH>(lds, R, a.X, l0, &l1, ACT_NONE, NO16, 0, a.F, nullptr, 0, row0, nrows, si);
    norm_fwd<P>(lds, a.F, a.Ha, rows, 1e-8f, a.CAT, 0, NO16, 0, NO32, nullptr, 0, nullptr, nullptr, row0, nrows);
    __syncthreads();
    // F overlaid H1 | H2: their zero padding columns (read by the GEMMs below
    // where the width is not a multiple of 32 PD) are restored before the
    // epilogues write H1 / H2 (a fast wave's epilogue may start while another
    // wave still zeroes: the barrier orders them)
    if (a.F.off == a.H1.off) {
        zero_lds(lds + a.H1.off, a.H2.off + rows * a.H2.ld * 2 - a.H1.off);
        __syncthreads();
    }
    layer_fwd<P, RT, TH>(lds, R, a.CAT, l1, &l2, a.act_actor, a.H1, 0, NO32, nullptr, 0, row0, nrows, si);
    layer_fwd<P, RT, TH>(lds, R, a.H1, l2, (const Lin *)nullptr, a.act_actor, a.H2, 0, NO32, nullptr, 0, row0, nrows, si);
    if constexpr (RT == 1) {
        layer_thin_fwd<P, THIN_NC>(lds, a.H2, l3, a.TW, ACT_TANH, a.FT, rows, nullptr, 0, row0, nrows, si);
    } else {  // thin products per 16-row tile, then bias + tanh over all rows
        FSTAMP(si);
#pragma unroll
        for (int t = 0; t < RT; ++t) thin<P, THIN_NC>(lds, rows_of(a.H2, t), 0, l3.K, a.TW, a.A, rows_of(a.FT, t), 1.f);
        __syncthreads();
        for (int k = threadIdx.x; k < rows * a.A; k += NTH) {
            const int row = k / a.A, c = k - row * a.A;
            *p32(lds, a.FT, row, c) = act_fwd(ACT_TANH, *p32(lds, a.FT, row, c) + ldg(l3.b + c));
        }
        __syncthreads();
    }
}

// noise_rows' sibling for a noise term that is already scaled (a coloured
// sequence per env: td7f_select_seq, td7f_select_multi_seq): global row R =
// row0 + row of the fp32 actions a gets e = seq[R][min(t[R], Lmax - 1)][c],
// clamped to +-clip when clip > 0; out = clamp(a + e, -1, 1) * scale.  Ends
// with a barrier, no ticket.
__device__ __forceinline__ void seq_rows(char *lds, R32 a, int A, int rows, int row0, int rend, const float *seq,
                                         const int *t, int Lmax, float clip, float scale, float *out) {
    for (int k = threadIdx.x; k < rows * A; k += NTH) {
        const int row = k / A, c = k - row * A, R = row0 + row;
        if (R < rend) {
            const int tt = min(max(ldg(t + R), 0), Lmax - 1);
            float e = ldg(seq + ((size_t)R * Lmax + tt) * A + c);
            if (clip > 0.f) e = fminf(fmaxf(e, -clip), clip);
            stg(out + (size_t)R * A + c, fminf(fmaxf(*p32(lds, a, row, c) + e, -1.0f), 1.0f) * scale);
        }
    }
    __syncthreads();
}

// The shape checks and the LDS plan of a select launch with `rows` rows per
// workgroup (obs, n, out and nz are the caller's); lds_bytes: the images' size.
// EXO_OK or EXO_EINVAL.
inline int select_plan(int prec, const int32_t *act, const td7f_lin *enc, const td7f_lin *actor, int rows,
                       SelectPlan &a, int &lds_bytes) {
    const int kd = kd_of(prec);
    a.act_enc = act[0];
    a.act_actor = act[1];
    a.S = enc[0].n_in;
    a.A = actor[3].n_out;
    a.Z = enc[2].n_out;
    a.Ha = actor[0].n_out;
    if (actor[0].n_in != a.S || actor[1].n_in != a.Ha + a.Z || a.A > THIN_NC || a.S > NTH) return EXO_EINVAL;
    const int hmax = std::max(enc[0].n_out, std::max(enc[1].n_out, std::max(a.Ha, actor[1].n_out)));
    Bump b;
    a.X = b.r16(rows, ld16(a.S, kd));
    a.H1 = b.r16(rows, ld16(hmax, kd));
    a.H2 = b.r16(rows, ld16(hmax, kd));
    const int fld = std::max(std::max(a.Z, a.Ha), 16);
    if (rows * fld * 4 <= a.H2.off + rows * a.H2.ld * 2 - a.H1.off) {
        a.F = R32{a.H1.off, fld};  // overlays H1 | H2 (both dead whenever F is written)
    } else {
        a.F = b.r32(rows, fld);
    }
    a.CAT = b.r16(rows, ld16(a.Ha + a.Z, kd));
    a.TW = b.r32(THIN_NC, actor[3].n_in);
    a.FT = b.r32(rows, 16);
    lds_bytes = b.off;
    return EXO_OK;
}

}  // namespace td7f
