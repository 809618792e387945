// td7_fused_multi.hip -- select_action of several policies in one launch.
//
//   td7f_select_multi : Agent.select_action (Agent/TD7_multi_agent.py:192-209,
//                       Agent/TD7_multi_agent_Pink_noise.py:212-214) for npol
//                       policies at once: policy p acts on the contiguous rows
//                       [seg[p], seg[p+1]) of obs.
//
// An evaluation of K policies over a few hundred envs each is K launches of a
// few dozen workgroups on 256 CUs; here the K row ranges are one grid.  The
// per-row arithmetic is select_kernel's (td7_fused.hip, 16-row tiles), built
// from the same blocks of td7_fused.h; what differs is where a workgroup gets
// its work from:
//
//   tile table   int32 [ntiles][3] = (policy, row0, row_end), indexed by
//                blockIdx.x.  A tile never straddles a segment (a workgroup
//                streams ONE policy's weights): a segment of len rows has
//                ceil(len / 16) tiles, the last one ragged.  row_end plays the
//                part select_kernel's a.n plays: rows >= row_end are neither
//                read nor written.
//   policy table td7f_lin [npol][7] = zs1..zs3, l0..l3 of each policy, in
//                device memory (seven Lins x 15 policies do not fit the kernel
//                arguments).  Pointers and shapes only: repacking a policy's
//                weights in place keeps it valid.
//
// Both tables are read with wave-uniform (scalar) loads: the addresses depend
// on blockIdx.x alone and nothing in the kernel stores to global memory before
// its last stage.
//
//   td7f_select_multi_noise : the same launch with one exploration-noise state
//                       PER POLICY (sigma, clip, decay, Philox stream), for
//                       collecting data from many behaviour policies at once:
//
//   noise table  td7f_noise_row [npol] in device memory: key, pointers to the
//                policy's call counter and sigma, sigma_dec, clip.  The
//                immutable fields are read wave-uniform like the other tables;
//                *sigma and *counter, which the launch writes, with ordinary
//                loads (noise_rows).
//   seg          int32 [npol + 1], a device copy: the Philox element of row r
//                of policy p is (r - seg[p]) * A + c, so what a policy draws
//                depends neither on its neighbours nor on where its segment
//                starts -- its rows equal its own td7f_select, noise included.
//   ticket       one word for the launch: the last workgroup out advances
//                every policy with a non-empty segment (thread k policy k).
//
//   td7f_select_multi_seq : the same launch with a coloured noise sequence per
//                       env (TD7_multi_agent_Pink_noise.py:203-228): the noise
//                       term of row r is column t[r] of its row of the table
//                       td7f_pink_advance (td7_pink.hip) keeps, already scaled
//                       by sigma; the ticket advances sigma only, no Philox
//                       counter moves.
#include "td7_fused.h"

#include <algorithm>

namespace td7f {

struct SelectMultiArgs {
    const td7f_lin *pol;  // device [npol][7]
    const int *tiles;     // device [ntiles][3]
    int act_enc, act_actor;
    const float *obs;
    int S, A, Z, Ha;
    float *out;
    Noise nz;
    int noisy;    // 0: deterministic (nz unused, no noise state touched)
    float scale;  // deterministic mode's max_action
    R16 X, H1, H2, CAT;
    R32 F, TW, FT;
    int lds_bytes;
};

// a wave-uniform 32-bit word as a scalar (the compiler folds it when the load
// already is one)
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
template <typename T>
__device__ __forceinline__ T *uni_ptr(const uint32_t *w) {
    return (T *)(uintptr_t)((unsigned long long)uni(w[0]) | ((unsigned long long)uni(w[1]) << 32));
}
// layer i of policy `pol` from the policy table (td7f_lin is 14 words)
__device__ __forceinline__ Lin lin_at(const td7f_lin *tab, int pol, int i) {
    static_assert(sizeof(td7f_lin) == 56, "td7f_lin: 3 pointers, 4 ints, pointer, int64");
    const uint32_t *p = (const uint32_t *)(tab + (size_t)pol * 7 + i);
    uint32_t w[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) w[k] = ldg(p + k);
    Lin L;
    L.wf = uni_ptr<const u32x4>(w);
    L.wb = uni_ptr<const u32x4>(w + 2);
    L.b = uni_ptr<const float>(w + 4);
    L.N = (int)uni(w[6]);
    L.K = (int)uni(w[7]);
    L.ksf = (int)uni(w[8]);
    L.ksb = (int)uni(w[9]);
    L.w = uni_ptr<const float>(w + 10);
    L.ldw = (long)((unsigned long long)uni(w[12]) | ((unsigned long long)uni(w[13]) << 32));
    return L;
}

// the tile (policy, row0, row_end) of blockIdx.x
__device__ __forceinline__ void tile_at(const int *tiles, int &pol, int &row0, int &rend) {
    const int *tp = tiles + 3 * (size_t)blockIdx.x;
    pol = (int)uni((uint32_t)ldg(tp));
    row0 = (int)uni((uint32_t)ldg(tp + 1));
    rend = (int)uni((uint32_t)ldg(tp + 2));
}

// select_kernel<P, TH, 1, 0>'s networks on the tile (pol, row0, rend): leaves
// tanh(l3(...)) of the tile's rows in the fp32 region a.FT.
template <int P, int TH>
__device__ __forceinline__ void select_multi_rows(char *lds, const SelectMultiArgs &a, int pol, int row0, int rend) {
    constexpr int rows = TR;
    int si = 0;
    FSTAMP(si);
    const Lin zs1 = lin_at(a.pol, pol, 0), l3 = lin_at(a.pol, pol, 6);
    RowStage so;
    ThinStage<THIN_NC> tw;
    row_issue(so, a.obs, a.S, a.S, row0, rend);
    thin_issue(tw, l3.w, l3.ldw, 0, false, a.A, l3.K);
    Ring<TH> R;
    ring_fill<TH>(R, GDesc{zs1.wf, zs1.ksf, 0});
    zero_lds(lds, a.lds_bytes);
    __syncthreads();
    row_put16<P>(lds, so, a.X, 0, a.S, row0, rend);
    thin_put<P>(lds, tw, a.TW, a.A, l3.K);
    __syncthreads();
    // zs = fixed_encoder.zs(obs) (:93-97) -> CAT[:, Ha:Ha+Z]
    const Lin zs2 = lin_at(a.pol, pol, 1), zs3 = lin_at(a.pol, pol, 2), l0 = lin_at(a.pol, pol, 3);
    layer_fwd<P, 1, TH>(lds, R, a.X, zs1, &zs2, a.act_enc, a.H1, 0, NO32, nullptr, 0, row0, rend, si);
    layer_fwd<P, 1, TH>(lds, R, a.H1, zs2, &zs3, a.act_enc, a.H2, 0, NO32, nullptr, 0, row0, rend, si);
    layer_fwd<P, 1, TH>(lds, R, a.H2, zs3, &l0, ACT_NONE, NO16, 0, a.F, nullptr, 0, row0, rend, si);
    norm_fwd<P>(lds, a.F, a.Z, rows, 1e-8f, a.CAT, a.Ha, NO16, 0, NO32, nullptr, 0, nullptr, nullptr, row0, rend);
    __syncthreads();
    // actor (:72-77): AvgL1Norm(l0(s)) | zs -> l1 -> l2 -> tanh(l3)
    const Lin l1 = lin_at(a.pol, pol, 4), l2 = lin_at(a.pol, pol, 5);
    layer_fwd<P, 1, TH>(lds, R, a.X, l0, &l1, ACT_NONE, NO16, 0, a.F, nullptr, 0, row0, rend, si);
    norm_fwd<P>(lds, a.F, a.Ha, rows, 1e-8f, a.CAT, 0, NO16, 0, NO32, nullptr, 0, nullptr, nullptr, row0, rend);
    __syncthreads();
    // F overlaid H1 | H2: their zero padding columns restored (see select_kernel)
    if (a.F.off == a.H1.off) {
        zero_lds(lds + a.H1.off, a.H2.off + rows * a.H2.ld * 2 - a.H1.off);
        __syncthreads();
    }
    layer_fwd<P, 1, TH>(lds, R, a.CAT, l1, &l2, a.act_actor, a.H1, 0, NO32, nullptr, 0, row0, rend, si);
    layer_fwd<P, 1, TH>(lds, R, a.H1, l2, (const Lin *)nullptr, a.act_actor, a.H2, 0, NO32, nullptr, 0, row0, rend, si);
    layer_thin_fwd<P, THIN_NC>(lds, a.H2, l3, a.TW, ACT_TANH, a.FT, rows, nullptr, 0, row0, rend, si);
}

// select_kernel<P, TH, 1, 0> on the tile (policy, row0, row_end) of blockIdx.x.
template <int P, int TH>
__global__ __launch_bounds__(NTH) void select_multi_kernel(SelectMultiArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int rows = TR;
    int pol, row0, rend;
    tile_at(a.tiles, pol, row0, rend);
    select_multi_rows<P, TH>(lds, a, pol, row0, rend);
    if (a.noisy) {
        // one noise state for the launch: the Philox element is the global
        // row's, the last workgroup out takes the ticket
        noise_rows<P>(lds, a.FT, a.A, rows, row0, rend, a.nz, a.out, NO16, 0, NO16, 0, true);
        return;
    }
    for (int k = threadIdx.x; k < rows * a.A; k += NTH) {
        const int row = k / a.A, c = k - row * a.A;
        if (row0 + row < rend)
            stg(a.out + (size_t)(row0 + row) * a.A + c, fminf(fmaxf(*p32(lds, a.FT, row, c), -1.0f), 1.0f) * a.scale);
    }
}

// ---- one noise state per policy (td7f_select_multi_noise)
struct SelectMultiNoiseArgs {
    SelectMultiArgs s;          // s.nz / s.noisy unused
    const td7f_noise_row *nzt;  // device [npol]
    const int *seg;             // device [npol + 1]
    uint32_t *ticket;
    const float *z;  // given standard normals [n][A] (null: Philox)
    int npol;
};

// row `pol` of the noise table as a Noise (td7f_noise_row is 10 words); only
// *sigma and *counter change during a launch, and noise_rows loads those
__device__ __forceinline__ Noise noise_at(const td7f_noise_row *tab, int pol, float scale, const float *z) {
    static_assert(sizeof(td7f_noise_row) == 40, "td7f_noise_row: u64, 2 x u32, 2 pointers, 2 floats");
    const uint32_t *p = (const uint32_t *)(tab + pol);
    uint32_t w[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) w[k] = ldg(p + k);
    Noise nz;
    nz.seed = (unsigned long long)uni(w[0]) | ((unsigned long long)uni(w[1]) << 32);
    nz.tag = uni(w[2]);
    nz.counter = uni_ptr<unsigned long long>(w + 4);
    nz.ticket = nullptr;
    nz.sigma = uni_ptr<float>(w + 6);
    nz.sigma_dec = __uint_as_float(uni(w[8]));
    nz.clip = __uint_as_float(uni(w[9]));
    nz.scale = scale;
    nz.z = z;
    nz.dec_count = nullptr;
    return nz;
}

// select_multi_kernel's rows with policy pol's own noise (noise_rows, Philox
// elements counted from seg[pol]); the last workgroup out advances the policies.
template <int P, int TH>
__global__ __launch_bounds__(NTH) void select_multi_noise_kernel(SelectMultiNoiseArgs m) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int rows = TR;
    const SelectMultiArgs &a = m.s;
    int pol, row0, rend;
    tile_at(a.tiles, pol, row0, rend);
    select_multi_rows<P, TH>(lds, a, pol, row0, rend);
    // noise_rows as it stands, on the segment as a tensor of its own: with the
    // rows counted from seg0 its element (row * A + c) is the segment-local
    // one, and out / z moved to the segment's first row put it back
    const int seg0 = (int)uni((uint32_t)ldg(m.seg + pol));
    const size_t off = (size_t)seg0 * a.A;
    const Noise nz = noise_at(m.nzt, pol, a.scale, m.z ? m.z + off : nullptr);
    noise_rows<P>(lds, a.FT, a.A, rows, row0 - seg0, rend - seg0, nz, a.out + off, NO16, 0, NO16, 0, false);
    // (noise_rows ended with a barrier: every thread of this workgroup has
    // read its sigma and counter, and the LDS images are dead)
    int *last = (int *)lds;
    if (threadIdx.x == 0) {
        __threadfence();
        *last = atomicAdd(m.ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!*last) return;
    // every workgroup has read its policy's state before its ticket: advance
    // the policies that acted, thread k policy k (vector lanes, plain stores)
    for (int k = threadIdx.x; k < m.npol; k += NTH) {
        if (ldg(m.seg + k + 1) <= ldg(m.seg + k)) continue;
        const td7f_noise_row *r = m.nzt + k;
        float *sg = ldg(&r->sigma);
        unsigned long long *cnt = ldg(&r->counter);
        *sg = ldg(sg) - ldg(&r->sigma_dec);
        if (!m.z) *cnt = ldg(cnt) + 1ull;
    }
    if (threadIdx.x == 0) *m.ticket = 0u;
}

// ---- a coloured sequence per env (td7f_select_multi_seq)
struct SelectMultiSeqArgs {
    SelectMultiArgs s;          // s.nz / s.noisy unused
    const td7f_noise_row *nzt;  // device [npol]: sigma, sigma_dec, clip (no Philox state is touched)
    const int *seg;             // device [npol + 1]
    uint32_t *ticket;
    const float *seq;  // [n][Lmax][A], td7f_pink_advance's table
    const int *t;      // [n] step index of each env's episode
    int Lmax, npol;
};

// noise_rows' sibling for a noise term that is already scaled: global row R =
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

// select_multi_kernel's rows plus each env's own column of its coloured
// sequence; the last workgroup out advances sigma of the policies with rows.
template <int P, int TH>
__global__ __launch_bounds__(NTH) void select_multi_seq_kernel(SelectMultiSeqArgs m) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int rows = TR;
    const SelectMultiArgs &a = m.s;
    int pol, row0, rend;
    tile_at(a.tiles, pol, row0, rend);
    select_multi_rows<P, TH>(lds, a, pol, row0, rend);
    const float clip = __uint_as_float(uni(ldg((const uint32_t *)(m.nzt + pol) + 9)));
    seq_rows(lds, a.FT, a.A, rows, row0, rend, m.seq, m.t, m.Lmax, clip, a.scale, a.out);
    // (seq_rows ended with a barrier: the LDS images are dead)
    int *last = (int *)lds;
    if (threadIdx.x == 0) {
        __threadfence();
        *last = atomicAdd(m.ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!*last) return;
    // sigma is read by td7f_pink_advance only, between launches: thread k policy k
    for (int k = threadIdx.x; k < m.npol; k += NTH) {
        if (ldg(m.seg + k + 1) <= ldg(m.seg + k)) continue;
        const td7f_noise_row *r = m.nzt + k;
        float *sg = ldg(&r->sigma);
        *sg = ldg(sg) - ldg(&r->sigma_dec);
    }
    if (threadIdx.x == 0) *m.ticket = 0u;
}

}  // namespace td7f

using namespace td7f;

extern "C" {

int td7f_multi_tiles(int32_t npol, const int32_t *seg, int32_t *tiles, int32_t cap) {
    if (npol <= 0 || !seg || seg[0] != 0 || cap < 0) return EXO_EINVAL;
    long nt = 0;
    for (int p = 0; p < npol; ++p) {
        if (seg[p + 1] < seg[p]) return EXO_EINVAL;
        for (int r = seg[p]; r < seg[p + 1]; r += TR, ++nt)
            if (tiles && nt < cap) {
                tiles[3 * nt] = p;
                tiles[3 * nt + 1] = r;
                tiles[3 * nt + 2] = std::min(r + TR, seg[p + 1]);
            }
    }
    if (nt > INT32_MAX) return EXO_ERANGE;
    return (int)nt;
}

// The host image of the policy table from the same enc / actor arrays the
// launch validates: the one place that fixes lin_at's layout on the host side.
int td7f_multi_policy_table(int32_t npol, const td7f_lin *enc, const td7f_lin *actor, td7f_lin *table) {
    if (npol <= 0 || !enc || !actor || !table) return EXO_EINVAL;
    for (int p = 0; p < npol; ++p) {
        for (int i = 0; i < 3; ++i) table[7 * (size_t)p + i] = enc[3 * (size_t)p + i];
        for (int i = 0; i < 4; ++i) table[7 * (size_t)p + 3 + i] = actor[4 * (size_t)p + i];
    }
    return EXO_OK;
}

// The host image of the noise table from per-policy td7f_noise structs: the
// one place that fixes noise_at's layout on the host side.
int td7f_multi_noise_table(int32_t npol, const td7f_noise *noise, td7f_noise_row *table) {
    if (npol <= 0 || !noise || !table) return EXO_EINVAL;
    for (int p = 0; p < npol; ++p) {
        // one ticket, one scale and one z serve the launch; no per-env decay count
        if (noise[p].z || noise[p].dec_count) return EXO_EINVAL;
        table[p] = td7f_noise_row{noise[p].seed, noise[p].tag, 0u, noise[p].counter, noise[p].sigma,
                                  noise[p].sigma_dec, noise[p].clip};
    }
    return EXO_OK;
}

}  // extern "C"

// td7f_select_multi's argument checks and LDS plan (select_impl's at RT = 1)
// into a; th: tiles per wave.  EXO_OK or the error to return.
static int multi_plan(int32_t prec, const int32_t *act, int32_t npol, const td7f_lin *enc, const td7f_lin *actor,
                      const void *policies_dev, const int32_t *seg, const int32_t *tiles_dev, int32_t ntiles,
                      const float *obs, int32_t n, float *out, float scale, SelectMultiArgs &a, int &th) {
    const bool prec_ok = prec == PREC_BF16 || prec == PREC_F16 || prec == PREC_F32;
    if (!prec_ok || !act || npol <= 0 || !enc || !actor || !policies_dev || !seg || !tiles_dev || !obs || !out ||
        n <= 0)
        return EXO_EINVAL;
    if (seg[0] != 0 || seg[npol] != n) return EXO_EINVAL;
    long nt = 0;
    for (int p = 0; p < npol; ++p) {
        if (seg[p + 1] < seg[p]) return EXO_EINVAL;
        nt += (seg[p + 1] - seg[p] + TR - 1) / TR;
    }
    if (nt != ntiles) return EXO_EINVAL;
    const int kd = kd_of(prec);
    th = 0;
    for (int p = 0; p < npol; ++p) {
        const td7f_lin *e = enc + 3 * (size_t)p, *c = actor + 4 * (size_t)p;
        td7f_lin all[7] = {e[0], e[1], e[2], c[0], c[1], c[2], c[3]};
        const int t = th_of(all, 7);
        if ((t != 4 && t != 5) || (p && t != th)) return EXO_EINVAL;
        th = t;
        // one LDS plan: every policy has policy 0's shape
        const td7f_lin *e0 = enc, *c0 = actor;
        for (int i = 0; i < 7; ++i) {
            const td7f_lin &x = i < 3 ? e[i] : c[i - 3], &y = i < 3 ? e0[i] : c0[i - 3];
            if (x.n_out != y.n_out || x.n_in != y.n_in || x.ksf != y.ksf) return EXO_EINVAL;
        }
    }
    a = SelectMultiArgs{};
    a.pol = (const td7f_lin *)policies_dev;
    a.tiles = tiles_dev;
    a.act_enc = act[0];
    a.act_actor = act[1];
    a.obs = obs;
    a.S = enc[0].n_in;
    a.A = actor[3].n_out;
    a.Z = enc[2].n_out;
    a.Ha = actor[0].n_out;
    if (actor[0].n_in != a.S || actor[1].n_in != a.Ha + a.Z || a.A > THIN_NC || a.S > NTH) return EXO_EINVAL;
    if ((long)n * a.A >= (1L << 31)) return EXO_ERANGE;  // the Philox element index is 32 bits
    a.out = out;
    a.scale = scale;
    // select_impl's plan at RT = 1
    const int rows = TR, hmax = std::max(enc[0].n_out, std::max(enc[1].n_out, std::max(a.Ha, actor[1].n_out)));
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
    a.lds_bytes = b.off;
    return EXO_OK;
}

extern "C" {

int td7f_select_multi(int32_t prec, const int32_t *act, int32_t npol, const td7f_lin *enc, const td7f_lin *actor,
                      const void *policies_dev, const int32_t *seg, const int32_t *tiles_dev, int32_t ntiles,
                      const float *obs, int32_t n, const td7f_noise *noise, float *out, float scale, void *stream) {
    SelectMultiArgs a;
    int th;
    const int rc = multi_plan(prec, act, npol, enc, actor, policies_dev, seg, tiles_dev, ntiles, obs, n, out, scale,
                              a, th);
    if (rc != EXO_OK) return rc;
    a.noisy = noise != nullptr;
    if (noise) a.nz = noise_of(*noise);
    return DISPATCH(prec, th, select_multi_kernel, dim3((unsigned)ntiles), a.lds_bytes, a, (hipStream_t)stream);
}

int td7f_select_multi_noise(int32_t prec, const int32_t *act, int32_t npol, const td7f_lin *enc,
                            const td7f_lin *actor, const void *policies_dev, const int32_t *seg,
                            const int32_t *tiles_dev, int32_t ntiles, const float *obs, int32_t n,
                            const td7f_noise_row *noise, const void *noise_dev, const int32_t *seg_dev,
                            uint32_t *ticket_dev, const float *z_dev, float *out, float scale, void *stream) {
    SelectMultiNoiseArgs m{};
    int th;
    const int rc = multi_plan(prec, act, npol, enc, actor, policies_dev, seg, tiles_dev, ntiles, obs, n, out, scale,
                              m.s, th);
    if (rc != EXO_OK) return rc;
    if (!noise || !noise_dev || !seg_dev || !ticket_dev) return EXO_EINVAL;
    for (int p = 0; p < npol; ++p) {
        if (!(noise[p].sigma_dec >= 0.f) || !(noise[p].clip >= 0.f)) return EXO_EINVAL;
        if (seg[p + 1] > seg[p] && (!noise[p].sigma || !noise[p].counter)) return EXO_EINVAL;
    }
    m.nzt = (const td7f_noise_row *)noise_dev;
    m.seg = seg_dev;
    m.ticket = ticket_dev;
    m.z = z_dev;
    m.npol = npol;
    return DISPATCH(prec, th, select_multi_noise_kernel, dim3((unsigned)ntiles), m.s.lds_bytes, m,
                    (hipStream_t)stream);
}

int td7f_select_multi_seq(int32_t prec, const int32_t *act, int32_t npol, const td7f_lin *enc, const td7f_lin *actor,
                          const void *policies_dev, const int32_t *seg, const int32_t *tiles_dev, int32_t ntiles,
                          const float *obs, int32_t n, const td7f_noise_row *noise, const void *noise_dev,
                          const int32_t *seg_dev, uint32_t *ticket_dev, const float *seq_dev, const int32_t *t_dev,
                          int32_t Lmax, float *out, float scale, void *stream) {
    SelectMultiSeqArgs m{};
    int th;
    const int rc = multi_plan(prec, act, npol, enc, actor, policies_dev, seg, tiles_dev, ntiles, obs, n, out, scale,
                              m.s, th);
    if (rc != EXO_OK) return rc;
    if (!noise || !noise_dev || !seg_dev || !ticket_dev || !seq_dev || !t_dev || Lmax <= 0) return EXO_EINVAL;
    for (int p = 0; p < npol; ++p) {
        if (!(noise[p].sigma_dec >= 0.f) || !(noise[p].clip >= 0.f)) return EXO_EINVAL;
        if (seg[p + 1] > seg[p] && !noise[p].sigma) return EXO_EINVAL;
    }
    m.nzt = (const td7f_noise_row *)noise_dev;
    m.seg = seg_dev;
    m.ticket = ticket_dev;
    m.seq = seq_dev;
    m.t = t_dev;
    m.Lmax = Lmax;
    m.npol = npol;
    return DISPATCH(prec, th, select_multi_seq_kernel, dim3((unsigned)ntiles), m.s.lds_bytes, m,
                    (hipStream_t)stream);
}

}  // extern "C"
