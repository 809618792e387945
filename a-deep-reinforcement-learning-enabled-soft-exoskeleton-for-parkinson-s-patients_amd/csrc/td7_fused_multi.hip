// td7_fused_multi.hip -- select_action of several policies in one launch.
//
//   td7f_select_multi : Agent.select_action (Agent/TD7_multi_agent.py:192-209,
//                       Agent/TD7_multi_agent_Pink_noise.py:212-214) for npol
//                       policies at once: policy p acts on the contiguous rows
//                       [seg[p], seg[p+1]) of obs.
//
// An evaluation of K policies over a few hundred envs each is K launches of a
// few dozen workgroups on 256 CUs; here the K row ranges are one grid.  The
// per-row arithmetic and the LDS plan are select_kernel's own (select_rows and
// select_plan of td7_select.h at 16-row tiles, the whole pass); what differs
// is where a workgroup gets its work from:
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
#include <algorithm>

#include "td7_select.h"

namespace td7f {

struct SelectMultiArgs {
    const td7f_lin *pol;  // device [npol][7]
    const int *tiles;     // device [ntiles][3]
    SelectPlan p;
    int lds_bytes;
    int noisy;    // 0: deterministic (p.nz unused, no noise state touched)
    float scale;  // deterministic mode's max_action
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

// select_rows' layers of policy `pol` from the policy table, loaded when asked for
struct TableLayers {
    const td7f_lin *tab;
    int pol;
    __device__ __forceinline__ Lin operator()(int i) const { return lin_at(tab, pol, i); }
};

// select_kernel<P, TH, 1, 0> on the tile (policy, row0, row_end) of blockIdx.x.
template <int P, int TH>
__global__ __launch_bounds__(NTH) void select_multi_kernel(SelectMultiArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int rows = TR;
    int pol, row0, rend;
    tile_at(a.tiles, pol, row0, rend);
    select_rows<P, TH, 1, 0>(lds, a.p, a.lds_bytes, row0, rend, nullptr, TableLayers{a.pol, pol});
    const int A = a.p.A;
    if (a.noisy) {
        // one noise state for the launch: the Philox element is the global
        // row's, the last workgroup out takes the ticket
        noise_rows<P>(lds, a.p.FT, A, rows, row0, rend, a.p.nz, a.p.out, NO16, 0, NO16, 0, true);
        return;
    }
    for (int k = threadIdx.x; k < rows * A; k += NTH) {
        const int row = k / A, c = k - row * A;
        if (row0 + row < rend)
            stg(a.p.out + (size_t)(row0 + row) * A + c, fminf(fmaxf(*p32(lds, a.p.FT, row, c), -1.0f), 1.0f) * a.scale);
    }
}

// ---- noise per policy: what td7f_select_multi_noise and td7f_select_multi_seq share
struct PerPolicyArgs {
    SelectMultiArgs s;          // s.p.nz / s.noisy unused
    const td7f_noise_row *nzt;  // device [npol]
    const int *seg;             // device [npol + 1]
    uint32_t *ticket;
    int npol;
};

// The end of a per-policy launch, called after a barrier that left the LDS
// images dead and every thread of this workgroup past its reads of its
// policy's state: the last workgroup out advances the policies that acted
// (sigma; with `counter` the Philox call counter too), thread k policy k
// (vector lanes, plain stores).
__device__ __forceinline__ void advance_policies(char *lds, const PerPolicyArgs &m, bool counter) {
    int *last = (int *)lds;
    if (threadIdx.x == 0) {
        __threadfence();
        *last = atomicAdd(m.ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!*last) return;
    for (int k = threadIdx.x; k < m.npol; k += NTH) {
        if (ldg(m.seg + k + 1) <= ldg(m.seg + k)) continue;
        const td7f_noise_row *r = m.nzt + k;
        float *sg = ldg(&r->sigma);
        *sg = ldg(sg) - ldg(&r->sigma_dec);
        if (counter) {
            unsigned long long *cnt = ldg(&r->counter);
            *cnt = ldg(cnt) + 1ull;
        }
    }
    if (threadIdx.x == 0) *m.ticket = 0u;
}

// ---- one noise state per policy (td7f_select_multi_noise)
struct SelectMultiNoiseArgs {
    PerPolicyArgs pp;
    const float *z;  // given standard normals [n][A] (null: Philox)
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
    const SelectMultiArgs &a = m.pp.s;
    int pol, row0, rend;
    tile_at(a.tiles, pol, row0, rend);
    select_rows<P, TH, 1, 0>(lds, a.p, a.lds_bytes, row0, rend, nullptr, TableLayers{a.pol, pol});
    // noise_rows as it stands, on the segment as a tensor of its own: with the
    // rows counted from seg0 its element (row * A + c) is the segment-local
    // one, and out / z moved to the segment's first row put it back
    const int seg0 = (int)uni((uint32_t)ldg(m.pp.seg + pol));
    const size_t off = (size_t)seg0 * a.p.A;
    const Noise nz = noise_at(m.pp.nzt, pol, a.scale, m.z ? m.z + off : nullptr);
    noise_rows<P>(lds, a.p.FT, a.p.A, rows, row0 - seg0, rend - seg0, nz, a.p.out + off, NO16, 0, NO16, 0, false);
    // (noise_rows ended with a barrier, after the reads of sigma and counter)
    advance_policies(lds, m.pp, !m.z);
}

// ---- a coloured sequence per env (td7f_select_multi_seq)
struct SelectMultiSeqArgs {
    PerPolicyArgs pp;  // of pp.nzt: sigma, sigma_dec, clip (no Philox state is touched)
    const float *seq;  // [n][Lmax][A], td7f_pink_advance's table
    const int *t;      // [n] step index of each env's episode
    int Lmax;
};

// select_multi_kernel's rows plus each env's own column of its coloured
// sequence (seq_rows, td7_select.h); the last workgroup out advances sigma of
// the policies with rows.
template <int P, int TH>
__global__ __launch_bounds__(NTH) void select_multi_seq_kernel(SelectMultiSeqArgs m) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int rows = TR;
    const SelectMultiArgs &a = m.pp.s;
    int pol, row0, rend;
    tile_at(a.tiles, pol, row0, rend);
    select_rows<P, TH, 1, 0>(lds, a.p, a.lds_bytes, row0, rend, nullptr, TableLayers{a.pol, pol});
    const float clip = __uint_as_float(uni(ldg((const uint32_t *)(m.pp.nzt + pol) + 9)));
    seq_rows(lds, a.p.FT, a.p.A, rows, row0, rend, m.seq, m.t, m.Lmax, clip, a.scale, a.p.out);
    // (seq_rows ended with a barrier; sigma is read by td7f_pink_advance only,
    // between launches)
    advance_policies(lds, m.pp, false);
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

// td7f_select_multi's argument checks and LDS plan (select_plan for policy 0
// at 16 rows) into a; th: tiles per wave.  EXO_OK or the error to return.
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
    if (select_plan(prec, act, enc, actor, TR, a.p, a.lds_bytes) != EXO_OK) return EXO_EINVAL;
    if ((long)n * a.p.A >= (1L << 31)) return EXO_ERANGE;  // the Philox element index is 32 bits
    a.p.obs = obs;
    a.p.n = n;
    a.p.out = out;
    a.scale = scale;
    return EXO_OK;
}

// ... and, after them, a per-policy launch's: the host image of the noise
// table (`counter`: a policy that acts needs a Philox call counter) into m
static int per_policy_plan(int32_t npol, const int32_t *seg, const td7f_noise_row *noise, const void *noise_dev,
                           const int32_t *seg_dev, uint32_t *ticket_dev, bool counter, PerPolicyArgs &m) {
    if (!noise || !noise_dev || !seg_dev || !ticket_dev) return EXO_EINVAL;
    for (int p = 0; p < npol; ++p) {
        if (!(noise[p].sigma_dec >= 0.f) || !(noise[p].clip >= 0.f)) return EXO_EINVAL;
        if (seg[p + 1] > seg[p] && (!noise[p].sigma || (counter && !noise[p].counter))) return EXO_EINVAL;
    }
    m.nzt = (const td7f_noise_row *)noise_dev;
    m.seg = seg_dev;
    m.ticket = ticket_dev;
    m.npol = npol;
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
    if (noise) a.p.nz = noise_of(*noise);
    return DISPATCH(prec, th, select_multi_kernel, dim3((unsigned)ntiles), a.lds_bytes, a, (hipStream_t)stream);
}

int td7f_select_multi_noise(int32_t prec, const int32_t *act, int32_t npol, const td7f_lin *enc,
                            const td7f_lin *actor, const void *policies_dev, const int32_t *seg,
                            const int32_t *tiles_dev, int32_t ntiles, const float *obs, int32_t n,
                            const td7f_noise_row *noise, const void *noise_dev, const int32_t *seg_dev,
                            uint32_t *ticket_dev, const float *z_dev, float *out, float scale, void *stream) {
    SelectMultiNoiseArgs m{};
    int th;
    int rc = multi_plan(prec, act, npol, enc, actor, policies_dev, seg, tiles_dev, ntiles, obs, n, out, scale,
                        m.pp.s, th);
    if (rc == EXO_OK) rc = per_policy_plan(npol, seg, noise, noise_dev, seg_dev, ticket_dev, true, m.pp);
    if (rc != EXO_OK) return rc;
    m.z = z_dev;
    return DISPATCH(prec, th, select_multi_noise_kernel, dim3((unsigned)ntiles), m.pp.s.lds_bytes, m,
                    (hipStream_t)stream);
}

int td7f_select_multi_seq(int32_t prec, const int32_t *act, int32_t npol, const td7f_lin *enc, const td7f_lin *actor,
                          const void *policies_dev, const int32_t *seg, const int32_t *tiles_dev, int32_t ntiles,
                          const float *obs, int32_t n, const td7f_noise_row *noise, const void *noise_dev,
                          const int32_t *seg_dev, uint32_t *ticket_dev, const float *seq_dev, const int32_t *t_dev,
                          int32_t Lmax, float *out, float scale, void *stream) {
    SelectMultiSeqArgs m{};
    int th;
    int rc = multi_plan(prec, act, npol, enc, actor, policies_dev, seg, tiles_dev, ntiles, obs, n, out, scale,
                        m.pp.s, th);
    if (rc == EXO_OK) rc = per_policy_plan(npol, seg, noise, noise_dev, seg_dev, ticket_dev, false, m.pp);
    if (rc != EXO_OK) return rc;
    if (!seq_dev || !t_dev || Lmax <= 0) return EXO_EINVAL;
    m.seq = seq_dev;
    m.t = t_dev;
    m.Lmax = Lmax;
    return DISPATCH(prec, th, select_multi_seq_kernel, dim3((unsigned)ntiles), m.pp.s.lds_bytes, m,
                    (hipStream_t)stream);
}

}  // extern "C"
