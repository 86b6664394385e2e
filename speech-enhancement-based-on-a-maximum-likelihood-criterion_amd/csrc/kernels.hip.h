// kernels.hip.h -- hand-written gfx950 (CDNA4) kernels for the ML-GGD DNN trainer.
//
// Replaces the reference's DevFunc.cu kernels + cuBLAS sgemm calls on the train/CV path
// (Train_code_ML_GGD/DevFunc.cu, DevFunc.h:49-87, call sites BP_GPU.cu:334-438,467-509).
//
// Device data layout (see DESIGN.md "HBM layout"): every unit dimension is padded to a
// multiple of 32 (Kp, Np) and the minibatch to Bp = ceil32(B); pad regions are kept at
// exactly 0 so the GEMM main loops need no masks.  Activations are kept in BOTH layouts:
//   Yt [units][Bp]  (frame index contiguous)  -> operand of the forward / dX MFMAs
//   Y  [Bp][units]  (unit index contiguous)   -> operand of the dW MFMAs
// so that every MFMA operand fragment (lane = non-reduction index) is a coalesced 128-byte
// row segment.  Weights stay in the reference's [in][out] row-major order (padded).
//
// All GEMMs use v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain, 64 FLOP/clk/SIMD).
// Fragment maps (cdna_hip_programming.md section 3): A: lane l holds A[i=l&31][k=l>>5];
// B: lane l holds B[k=l>>5][j=l&31]; C/D reg r: row=(r&3)+8*(r>>2)+4*(l>>5), col=l&31.
#pragma once
#include <hip/hip_runtime.h>
#include "nat_rule.h"
#include "asym_rule.h"
#include "scale_rule.h"
#include "adam_rule.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// Workgroups that share a weight tile (the b_tiles frame-blocks of one unit-tile) are given
// ids that are equal mod 8 and adjacent in dispatch order, so they land on one XCD and the
// tile is fetched from HBM/MALL once and re-read from that XCD's L2 (speed only; any
// placement is correct).
// x / d and x % d for a divisor the host has looked at: shift >= 0 means d == 1 << shift.  (A runtime integer
// division is ~40 scalar instructions on this ISA, a 64-bit one ~200: the prologue of the forward kernel spent
// ~1 us -- a tenth of the launch -- dividing before its first load was issued.)
__device__ __forceinline__ void divmod_by(int x, int d, int shift, int &q, int &r) {
    if (shift >= 0) {
        q = x >> shift;
        r = x & (d - 1);
    } else {
        q = (int)((unsigned)x / (unsigned)d);
        r = x - q * d;
    }
}
__device__ __forceinline__ void tile_of_block(int id, int u_tiles, int b_tiles, int b_shift, int &ut, int &bt, int map = 0) {
    if ((u_tiles & 7) == 0 && map != 2) {
        const int xcd = id & 7, slot = id >> 3;
        // map 0: an XCD owns unit tiles xcd, xcd+8, ...; map 1: a contiguous run of u_tiles/8 tiles
        int q;
        divmod_by(slot, b_tiles, b_shift, q, bt);
        ut = map == 1 ? xcd * (u_tiles >> 3) + q : xcd + 8 * q;
    } else {
        divmod_by(id, b_tiles, b_shift, ut, bt);
    }
}

template <int U>
struct FragU {
    float a[U];
    float b[U];
};

// Buffer-resource loads: per-lane byte offset in a VGPR (fixed for the whole kernel), the
// moving part of the address in an SGPR, out-of-range reads return 0 (hardware range check).
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void *p, size_t bytes) {
    const unsigned n = bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)bytes;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)n, 0x00020000);
}
__device__ __forceinline__ float bload(rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ float4 bload4(rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
// Diagnostic phase stamps (100 MHz wall clock).  `stamps` is nullptr in every normal launch;
// mlggd_debug_stamp_select() passes a buffer for ONE launch and the values go nowhere else.
__device__ __forceinline__ void stamp(long long *stamps, int slot, int bid = -1) {
    if (stamps != nullptr && threadIdx.x == 0) {
        stamps[(size_t)(bid < 0 ? (int)blockIdx.x : bid) * 8 + slot] = (long long)__builtin_amdgcn_s_memrealtime();
    }
}
// shader-clock counter next to the wall-clock stamp: (slot+1 - slot'+1) / (slot - slot') * 100 MHz is
// the clock the workgroup actually ran at
__device__ __forceinline__ void stamp_clk(long long *stamps, int slot, int bid) {
    if (stamps != nullptr && threadIdx.x == 0) {
        stamps[(size_t)bid * 8 + slot] = (long long)__builtin_amdgcn_s_memrealtime();
        stamps[(size_t)bid * 8 + slot + 1] = (long long)__builtin_amdgcn_s_memtime();
    }
}
// wave index as a provably wave-uniform value (scalar branches, exact s_waitcnt counts)
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// ---------------------------------------------------------------------------------------
// The exponential of the sigmoid (kernSigmoid, DevFunc.cu:48: 1 / (1 + exp(-x)); CUDA's expf is a <= 2 ulp function of
// its own -- which bits it returns no source reading can settle).  This one is written out in IEEE operations ONLY --
// multiplies, adds, one floor, one float -> int conversion, two exact powers of two; no fused multiply-add (the build
// has -ffp-contract=off), no hardware transcendental -- so that oracle/mlggd_oracle.c `ora_exp_det` (the SAME
// statements, compiled by gcc) returns the same bits for every input, and a whole training run of a net whose loss
// needs no powf (MMSE; ML-GGD with beta = 1, the shipped objective) equals the oracle's MFMA-order twin BIT FOR BIT
// (tests/test_gpu_mfma_order.py).  Cody-Waite reduction x = n ln2 + r, |r| <= 0.35, degree-6 polynomial (the
// classic Cephes expf coefficients), scaled by 2^n in two exact steps.  Measured against float64 over 2.3e7 inputs
// (tests/test_oracle.py): <= 0.96 ulp (ocml's expf: 1 ulp, glibc's: 0.5); the sigmoid built on it <= 2.5 ulp,
// the same as with glibc's.  Below -85.5 it saturates at 7.4e-38 (1 + e rounds to 1 there long before).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float exp_det(float x0) {
    // (selects, not branches: the four elements of a thread stay one straight instruction stream -- 1 us per step)
    float x = x0 < -85.5f ? -85.5f : x0;  // n >= -123 below: y * 2^(n-1) stays a normal number
    x = x > 88.72283f ? 88.72283f : x;    // beyond it the result is +inf (selected at the end)
    x = x0 != x0 ? 0.0f : x;              // a NaN comes back as it is (selected at the end)
    const float fn = __builtin_floorf(1.44269504f * x + 0.5f);
    float r = x - fn * 0.693359375f;
    r = r - fn * -2.12194440e-4f;
    const float z = r * r;
    float p = 1.9875691500e-4f;
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    float y = p * z + r;
    y = y + 1.0f;
    const float e = (y * __builtin_bit_cast(float, ((int)fn + 126) << 23)) * 2.0f;  // 2^n as 2^(n-1) * 2: n = 128 has no float of its own
    return x0 != x0 ? x0 : x0 > 88.72283f ? __builtin_inff() : e;
}
__device__ __forceinline__ float sigmoid_det(float x) { return 1.0f / (1.0f + exp_det(-x)); }  // kernSigmoid, DevFunc.cu:48
// Two elements at a time: the SAME operations per element, issued as packed fp32 instructions (v_pk_mul_f32 /
// v_pk_add_f32 are two independent IEEE operations per lane) -- the forward epilogues' four sigmoids per thread in half the
// multiply / add instructions (-0.8 us per step in a same-box A/B); results are those of exp_det bit for bit
// (tests/test_gpu_loss_ulps.py compares both forms).
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2_t exp_det2(f32x2_t x0) {
    f32x2_t x;
    x.x = x0.x < -85.5f ? -85.5f : x0.x;
    x.y = x0.y < -85.5f ? -85.5f : x0.y;
    x.x = x.x > 88.72283f ? 88.72283f : x.x;
    x.y = x.y > 88.72283f ? 88.72283f : x.y;
    x.x = x0.x != x0.x ? 0.0f : x.x;
    x.y = x0.y != x0.y ? 0.0f : x.y;
    const f32x2_t t = x * 1.44269504f + 0.5f;
    f32x2_t fn;
    fn.x = __builtin_floorf(t.x);
    fn.y = __builtin_floorf(t.y);
    f32x2_t r = x - fn * 0.693359375f;
    r = r - fn * -2.12194440e-4f;
    const f32x2_t z = r * r;
    f32x2_t p = {1.9875691500e-4f, 1.9875691500e-4f};
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    f32x2_t y = p * z + r;
    y = y + 1.0f;
    f32x2_t sc;
    sc.x = __builtin_bit_cast(float, ((int)fn.x + 126) << 23);
    sc.y = __builtin_bit_cast(float, ((int)fn.y + 126) << 23);
    f32x2_t e = (y * sc) * 2.0f;
    e.x = x0.x != x0.x ? x0.x : x0.x > 88.72283f ? __builtin_inff() : e.x;
    e.y = x0.y != x0.y ? x0.y : x0.y > 88.72283f ? __builtin_inff() : e.y;
    return e;
}
// y = sigmoid(v + b) for the four values of a thread, 0 where `live` is false (pad units)
__device__ __forceinline__ float4 sigmoid_det4(float4 v, float b, bool live) {
    const f32x2_t lo = {-(v.x + b), -(v.y + b)}, hi = {-(v.z + b), -(v.w + b)};
    const f32x2_t e0 = exp_det2(lo) + 1.0f, e1 = exp_det2(hi) + 1.0f;
    float4 y;
    y.x = live ? 1.0f / e0.x : 0.0f;
    y.y = live ? 1.0f / e0.y : 0.0f;
    y.z = live ? 1.0f / e1.x : 0.0f;
    y.w = live ? 1.0f / e1.y : 0.0f;
    return y;
}
// The rectifier's counterpart (FWD_RELU): y = x where x = v + b is not negative, else +0; 0 where `live` is false.  A
// comparison and a select, not fmaxf: v_max_f32 returns the other operand for a NaN, and a diverged net must show in
// the log as it does with the sigmoid.  x itself is the fp32 sum the sigmoid's epilogue forms, nothing is fused into it.
__device__ __forceinline__ float relu_det(float x) { return (x < 0.0f) ? 0.0f : x; }
__device__ __forceinline__ float4 relu4(float4 v, float b, bool live) {
    float4 y;
    y.x = live ? relu_det(v.x + b) : 0.0f;
    y.y = live ? relu_det(v.y + b) : 0.0f;
    y.z = live ? relu_det(v.z + b) : 0.0f;
    y.w = live ? relu_det(v.w + b) : 0.0f;
    return y;
}
// Its derivative for the dX epilogues (ACT_RELU): the gradient passes where the unit fired, exactly +0 elsewhere -- a
// dropped unit (y == 0) gets none, as y (1 - y) gives for the sigmoid
__device__ __forceinline__ float drelu(float y, float dedy) { return (y > 0.0f) ? dedy : 0.0f; }

// The power of the loss chain (pow_or_self below; kernindex2 / kernfunc2, DevFunc.cu:219-227,468-489): pow_det, x^y (x >= 0) as exp(y log x) in IEEE DOUBLE operations only -- adds, multiplies,
// one division, one floor, exact bit manipulation; no fused multiply-add, no libm, no hardware transcendental -- so that
// oracle/mlggd_oracle.c `ora_pow_det` (the SAME statements, compiled by gcc) returns the same bits for every argument and
// the loss chain equals the oracle's MFMA-order twin bit for bit at EVERY beta, like the GEMMs and the sigmoid
// (tests/test_gpu_mfma_order.py: whole training runs).  log m = 2 atanh((m-1)/(m+1)) by its series on [sqrt(1/2), sqrt 2),
// exp by Cody-Waite reduction and its Taylor polynomial of degree 13: ~1e-15 relative in double, so the float result is
// the CORRECTLY ROUNDED power in all but 5 of a million cases (measured against 80-bit powl over 2.2e7 arguments,
// tests/test_oracle.py; glibc's powf: 640 of a million, ocml's: 110,000-230,000).  CUDA's powf is a 2-ulp function of its own.
__device__ __forceinline__ float pow_det(float xf, float yf) {
    if (xf != xf || yf != yf) return xf + yf;
    if (yf == 0.0f) return 1.0f;
    if (xf == 0.0f) return yf > 0 ? 0.0f : __builtin_inff();
    if (xf == __builtin_inff()) return yf > 0 ? __builtin_inff() : 0.0f;
    const double x = (double)xf, y = (double)yf;  // exact; a float denormal is a normal double
    const long long bits = __builtin_bit_cast(long long, x);
    int e = (int)((bits >> 52) & 0x7ff) - 1023;
    double m = __builtin_bit_cast(double, (bits & 0x000fffffffffffffLL) | 0x3ff0000000000000LL);  // [1, 2)
    if (m > 1.4142135623730951) { m = m * 0.5; e = e + 1; }                                        // [sqrt(1/2), sqrt 2)
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double p = 1.0 / 21.0;  // log m = 2 s (1 + z/3 + z^2/5 + ...), |s| <= 0.1716: z^10 / 21 < 2e-17
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0;
    const double lg = (2.0 * s) * p + (double)e * 0.6931471805599453;
    const double t = y * lg;
    if (t > 89.0) return __builtin_inff();
    if (t < -104.0) return 0.0f;
    const double fn = __builtin_floor(t * 1.4426950408889634 + 0.5);
    double r = t - fn * 0.6931471803691238;  // ln 2, high part (its trailing bits are zero: fn * high is exact)
    r = r - fn * 1.9082149292705877e-10;     // ln 2, low part
    double q = 1.0 / 6227020800.0;           // 1 / 13!
    q = q * r + 1.0 / 479001600.0;
    q = q * r + 1.0 / 39916800.0;
    q = q * r + 1.0 / 3628800.0;
    q = q * r + 1.0 / 362880.0;
    q = q * r + 1.0 / 40320.0;
    q = q * r + 1.0 / 5040.0;
    q = q * r + 1.0 / 720.0;
    q = q * r + 1.0 / 120.0;
    q = q * r + 1.0 / 24.0;
    q = q * r + 1.0 / 6.0;
    q = q * r + 0.5;
    q = q * r + 1.0;
    q = q * r + 1.0;
    const int n = (int)fn;  // in [-151, 129]: 2^n is a normal double
    return (float)(q * __builtin_bit_cast(double, (long long)(n + 1023) << 52));
}

// ---------------------------------------------------------------------------------------
// Forward GEMM + bias + sigmoid:   X^T[n][b] = sum_k W[k][n] * Yt_in[k][b]  (+ bias[n])
// replaces kernMultiCopy + cublasSgemm(N,N) + kernSigmoid (BP_GPU.cu:360-364, DevFunc.cu:36-51,
// 134-149).  One workgroup = one 32(n) x 32(b) output tile; its NW waves split the reduction
// K and are summed through LDS in wave order (deterministic).
//
// Operand path (measured, DESIGN.md "why 16-byte loads"): a 4-byte-per-lane vector load costs
// the CU's address unit as much as a 16-byte one, and two of them per MFMA cap this kernel at
// ~60 % of the MFMA rate.  So each wave stages its OWN 32-row chunk of both operands with
// 16-byte buffer loads (8 lanes per 128-byte row segment, 0.5 load instructions per MFMA)
// into a wave-private LDS tile and reads the MFMA fragments back with ds_read_b32 (lanes
// 0-31 = 32 consecutive floats, conflict-free).  LDS operations of one wave execute in
// order, so no barrier is needed between a wave's ds_write and its own ds_read.
// MODE FWD_SIGMOID: fused epilogue writes y=1/(1+expf(-x)) (0 for pad units) to Yt_out and Y_out.
// MODE FWD_SLAB   : inter-workgroup K split S (small output layers); writes raw partial sums
//                   slab[s][n][b]; the consumer adds the bias and the S slabs in order.
// MODE FWD_RELU   : FWD_SIGMOID with the rectifier y = (x < 0) ? 0 : x as the activation (relu4); same stores, same
//                   layouts.  The activation is a template parameter, never a run-time branch: the sigmoid
//                   instantiations compile from the statements they had before there was a choice.
// ---------------------------------------------------------------------------------------
enum { FWD_SIGMOID = 0, FWD_SLAB = 1, FWD_RELU = 2 };
enum { ACT_SIGMOID = 0, ACT_RELU = 1 };  // the dX kernels' switch; the values of MLGGD_ACT_* (include/mlggd.h)
// dx_body's other epilogues: the product is an RBM's reconstruction (rbm.hip.h), DxArgs.Yt_prev the visible bias c [Kp]
enum { ACT_VIS_LINEAR = 2, ACT_VIS_SIGMOID = 3 };

struct FwdArgs {
    const float *W, *Yt_in, *bias;
    float *Yt_out, *Y_out, *slab;
    int Kp, Np, Bp, N, n_tiles, b_tiles, S, map;
    int b_shift, s_shift;  // log2 of b_tiles / S when they are powers of two, else -1 (divmod_by)
    int yblk;              // 0: Y_out is row-major [Bp][Np]; > 0: blocked by owner (y_blocked_base)
};
// The row-major activations Y [frame][unit] are what the dW kernels read -- and, data parallel, what a rank SENDS.  In
// the all-to-all form of the sharded update rank o only needs the units of ITS block of weight
// rows from every other rank, so the producer writes Y blocked by owner: [unit block o][frame][unit within the block]
// (block width yblk, a multiple of 64, so a 32- or 64-wide output tile never straddles two blocks); each block is then
// one contiguous message, and what arrives is a plain [world x frames][yblk] matrix for the dW tile records.
// u0: first unit of the tile.  Returns the offset of (frame 0, unit u0); frames are yblk floats apart.
__device__ __forceinline__ size_t y_blocked_base(int u0, int yblk, int Bp) {
    const int blk = (int)((unsigned)u0 / (unsigned)yblk);
    return (size_t)blk * Bp * yblk + (u0 - blk * yblk);
}
// LDS floats needed by fwd_body: staging / reduction tiles (two 8 KB tiles per wave) + the 32x36 transposition tile.
// One form is left -- 4 waves, main loop pipelined inside the wave with operands by LDS-DMA (PIPE 4) -- and the
// parameter lists are kept as they were, so that the kernels keep their names.
template <int NW, int PIPE> constexpr int fwd_lds_floats() {
    static_assert(NW == 4 && PIPE == 4, "the forward kernels have one form");
    return NW * 4096 + 32 * 36;
}

template <int MODE, int NW, int PIPE = 1>
__device__ __forceinline__ void fwd_body(const FwdArgs &A, const int bid, float *smem, long long *stamps) {
    static_assert(NW == 4 && PIPE == 4, "the forward kernels have one form");
    const float *__restrict__ W = A.W, *__restrict__ Yt_in = A.Yt_in, *__restrict__ bias = A.bias;
    float *__restrict__ Yt_out = A.Yt_out, *__restrict__ Y_out = A.Y_out, *__restrict__ slab = A.slab;
    const int Kp = A.Kp, Np = A.Np, Bp = A.Bp, N = A.N, n_tiles = A.n_tiles, b_tiles = A.b_tiles, S = A.S;
    // per wave: two tiles of [32 k rows][32] of W then [32 k rows][32] of Yt (8 KB each); the cross-wave
    // reduction buffer red[NW][1024] aliases the same storage after the main loop
    float(*tileT)[36] = reinterpret_cast<float(*)[36]>(smem + NW * 4096);
    stamp(stamps, 0, bid);
    stamp_clk(stamps, 4, bid);
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int i = lane & 31, h = lane >> 5;
    int id = bid, s = 0;
    // The slab form branches on its arguments (divmod_by) before it has used most of them, and the compiler then
    // fetches the rest only behind the branch: a second dependent round trip to kernel-argument memory in front of the
    // first operand load.  The empty asm names every argument the prologue needs, so all are requested in one group.
    if (MODE == FWD_SLAB)
        asm volatile("" ::"s"(W), "s"(Yt_in), "s"(slab), "s"(Kp), "s"(Np), "s"(Bp), "s"(N), "s"(n_tiles), "s"(b_tiles), "s"(S),
                     "s"(A.map), "s"(A.b_shift), "s"(A.s_shift));
    if (MODE == FWD_SLAB) divmod_by(bid, S, A.s_shift, id, s);
    int nt, bt;
    tile_of_block(id, n_tiles, b_tiles, A.b_shift, nt, bt, A.map);
    const int n0 = nt * 32, b0 = bt * 32;

    // k-pairs of this wave: slot = s*NW+wave of S*NW slots over Kp/2 pairs
    const int P = Kp >> 1;
    const int slot = s * NW + wave, nslots = S * NW;
    // floor(P * slot / nslots) in 32 bits (P * nslots < 2^31 for any layer this engine accepts); without slabs the
    // divisor is the compile-time wave count
    int p0, p1;
    if (MODE == FWD_SLAB) {
        p0 = (int)((unsigned)(P * slot) / (unsigned)nslots);
        p1 = (int)((unsigned)(P * (slot + 1)) / (unsigned)nslots);
    } else {
        p0 = (int)((unsigned)(P * wave) / (unsigned)NW);
        p1 = (int)((unsigned)(P * (wave + 1)) / (unsigned)NW);
    }
    const int npairs = p1 - p0;
    const int nch = (npairs + 15) >> 4;  // chunks of 16 pairs = 32 k rows

    const rsrc_t rW = make_rsrc(W, (size_t)Kp * Np * 4), rY = make_rsrc(Yt_in, (size_t)Kp * Bp * 4);
    const int r8 = lane >> 3, c4 = lane & 7;
    const int voW = (r8 * Np + n0 + 4 * c4) * 4, voY = (r8 * Bp + b0 + 4 * c4) * 4;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;

    // The epilogue's global operands (the bias of this thread's output elements) are fetched NOW: left alone the
    // compiler sinks the loads behind the last barrier, one after the other, and their L2 latency -- twice -- is the
    // tail of every launch (round 2: the ISA showed load -> exp -> store -> load -> exp -> store after the
    // reduction).  The empty asm with a "memory" clobber is a compiler-level fence the loads cannot be sunk across;
    // it does not use their values, so nothing waits for them until the epilogue does.  (A/B in one process: dX -0.2 ..
    // -0.3 us per launch, forward within noise: the loads hit L2.)
    // (bias_pre fed the epilogue of the 8- and 16-wave forms and nothing reads it since they went.  The statements
    // stayed so that retiring those forms moved no instruction: without them the compiler numbers two address registers
    // of every k_fwd the other way round, profiles/retired_arms_isa.txt.  A change that moves k_fwd's text anyway
    // can drop them.)
    constexpr int NT_ = 64 * NW, EPT_ = 1024 / NT_ > 0 ? 1024 / NT_ : 1;
    float bias_pre[EPT_];
#pragma unroll
    for (int q = 0; q < EPT_; q++) bias_pre[q] = MODE != FWD_SLAB ? bias[n0 + ((tid + NT_ * q) >> 5)] : 0.0f;
    const float bias_row = MODE != FWD_SLAB ? bias[n0 + (tid >> 3)] : 0.0f;  // a thread owns 4 frames of one unit
    asm volatile("" ::: "memory");

    // LDS-DMA form of the pipelined loop: a chunk goes global -> LDS directly (buffer_load ... lds, one wave-load = 8
    // rows of 128 B = 1 KB of the row-major tile), no staging registers, no ds_write.  Two tiles per wave: while the
    // MFMAs of chunk c run on registers, chunk c+2 is requested into the tile chunk c was read from (groups 0..3) and
    // the fragments of chunk c+1 are read from the other tile (groups 4..7) behind a counted vmcnt that leaves the
    // eight younger DMA instructions in flight.
    float *t0 = smem + wave * 4096, *t1 = t0 + 2048;
    const int endW = Kp * Np * 4, endY = Kp * Bp * 4;
    float fa[16], fb[16], ga[16], gb[16];
#define FWD_DMA1(T, C, Q)                                                          \
    {                                                                              \
        const int row0 = 2 * (p0 + 16 * (C));                                      \
        const bool live = (C) < nch;                                               \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (__attribute__((address_space(3))) void *)(T + (Q) * 256), 16, voW, \
                                                 live ? (row0 + 8 * (Q)) * Np * 4 : endW, 0, 0);        \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rY, (__attribute__((address_space(3))) void *)(T + 1024 + (Q) * 256), 16, voY, \
                                                 live ? (row0 + 8 * (Q)) * Bp * 4 : endY, 0, 0);        \
    }
#define FWD_RD4(T, NA, NB, Q)                                                      \
    {                                                                              \
        _Pragma("unroll") for (int u = 4 * (Q); u < 4 * (Q) + 4; u++) {            \
            NA[u] = (T)[h * 32 + i + u * 64];                                      \
            NB[u] = (T)[1024 + h * 32 + i + u * 64];                               \
        }                                                                          \
    }
    // chunk C on (FA, FB), read from tile TC one body ago; chunk C+1 is in tile TN (or landing); chunk C+2 -> TC
#define FWD_BODYD(FA, FB, NA, NB, TC, TN, C)                                       \
    {                                                                              \
        __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0): the fragment reads of TC have returned */ \
        _Pragma("unroll") for (int g = 0; g < 4; g++) {                            \
            acc = mfma32(FA[2 * g], FB[2 * g], acc);                               \
            acc = mfma32(FA[2 * g + 1], FB[2 * g + 1], acc);                       \
            FWD_DMA1(TC, (C) + 2, g);                                              \
            __builtin_amdgcn_sched_barrier(0);                                     \
        }                                                                          \
        __builtin_amdgcn_s_waitcnt(0x0F70 | 8); /* vmcnt(8): chunk C+1 has landed, chunk C+2 may be in flight */ \
        _Pragma("unroll") for (int g = 4; g < 8; g++) {                            \
            acc = mfma32(FA[2 * g], FB[2 * g], acc);                               \
            acc = mfma32(FA[2 * g + 1], FB[2 * g + 1], acc);                       \
            FWD_RD4(TN, NA, NB, g - 4);                                            \
            __builtin_amdgcn_sched_barrier(0);                                     \
        }                                                                          \
    }
#define FWD_DRAIND(FA, FB, CNT)                                                    \
    {                                                                              \
        _Pragma("unroll") for (int u = 0; u < 16; u++) {                           \
            if (u < (CNT)) acc = mfma32(FA[u], FB[u], acc);                        \
        }                                                                          \
    }
    if (nch > 0) {
        const int nfull = npairs >> 4, rem = npairs & 15;
#pragma unroll
        for (int q = 0; q < 4; q++) FWD_DMA1(t0, 0, q);
#pragma unroll
        for (int q = 0; q < 4; q++) FWD_DMA1(t1, 1, q);
        __builtin_amdgcn_s_waitcnt(0x0F70 | 8);
#pragma unroll
        for (int q = 0; q < 4; q++) FWD_RD4(t0, fa, fb, q);
        __builtin_amdgcn_sched_barrier(0);
        int c = 0;
        for (; c + 1 < nfull; c += 2) {
            FWD_BODYD(fa, fb, ga, gb, t0, t1, c);
            FWD_BODYD(ga, gb, fa, fb, t1, t0, c + 1);
        }
        if (c < nfull) {
            FWD_BODYD(fa, fb, ga, gb, t0, t1, c);
            FWD_DRAIND(ga, gb, rem);
        } else {
            FWD_DRAIND(fa, fb, rem);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70 | 0);  // nothing may still be landing in LDS when the reduction reuses it
    }
#undef FWD_DMA1
#undef FWD_RD4
#undef FWD_BODYD
#undef FWD_DRAIND

    stamp(stamps, 1, bid);
    // cross-wave reduction through LDS (aliases the staging tiles: wait for every wave)
    __syncthreads();
    float(*red)[1024] = reinterpret_cast<float(*)[1024]>(smem);
#pragma unroll
    for (int r = 0; r < 16; r++) red[wave][acc_row(r, lane) * 32 + i] = acc[r];
    __syncthreads();
    stamp(stamps, 2, bid);
    // 256 threads: a thread owns 4 consecutive frames of one unit.  The four partial tiles come in with one
    // ds_read_b128 each (added in wave order: deterministic), both output layouts leave as 16-byte stores
    // (11 LDS / memory instructions per thread instead of 32)
    const int row = tid >> 3, col4 = (tid & 7) * 4;
    float4 v4 = *reinterpret_cast<const float4 *>(&red[0][row * 32 + col4]);
#pragma unroll
    for (int w = 1; w < NW; w++) {
        const float4 p4 = *reinterpret_cast<const float4 *>(&red[w][row * 32 + col4]);
        v4.x += p4.x;
        v4.y += p4.y;
        v4.z += p4.z;
        v4.w += p4.w;
    }
    if (MODE == FWD_SLAB) {
        *reinterpret_cast<float4 *>(&slab[((size_t)s * Np + n0 + row) * Bp + b0 + col4]) = v4;
    } else {
        const int n = n0 + row;
        const float4 y4 = MODE == FWD_RELU ? relu4(v4, bias_row, n < N) : sigmoid_det4(v4, bias_row, n < N);  // kernSigmoid, DevFunc.cu:48
        *reinterpret_cast<float4 *>(&Yt_out[(size_t)n * Bp + b0 + col4]) = y4;
        tileT[col4][row] = y4.x;
        tileT[col4 + 1][row] = y4.y;
        tileT[col4 + 2][row] = y4.z;
        tileT[col4 + 3][row] = y4.w;
        __syncthreads();
        // thread -> frame row, 4 consecutive units
        const size_t yo = A.yblk ? y_blocked_base(n0, A.yblk, Bp) + (size_t)(b0 + row) * A.yblk + col4
                                 : (size_t)(b0 + row) * Np + n0 + col4;
        *reinterpret_cast<float4 *>(&Y_out[yo]) = *reinterpret_cast<const float4 *>(&tileT[row][col4]);
    }
    stamp(stamps, 3, bid);
    stamp_clk(stamps, 6, bid);
}

// ---------------------------------------------------------------------------------------
// Backward-data GEMM + sigmoid derivative:
//   dEdY^T[k][b] = sum_n W[k][n] * dEdXt[n][b] ;  dEdX_prev = (1-y)*y*dEdY
// replaces cublasSgemm(T,N) (BP_GPU.cu:430, DevFunc.h:49-63) + kernDsigmoid of the layer
// below (BP_GPU.cu:402, DevFunc.cu:53-71).  W is read with OLD values (launched before the
// update of the same layer).  Same structure as k_fwd (one 32x32 tile per workgroup, NW waves
// split the reduction n, wave-private LDS staging with 16-byte loads).  The reduction index n
// is the CONTIGUOUS index of W, so the W piece [32 k][64 n] is staged row-wise (16 lanes per
// 256-byte row segment) and the A fragments are read back transposed (row stride 66 floats:
// conflict-free ds_read_b64 giving two consecutive n per lane).
// ---------------------------------------------------------------------------------------
#define DX_LDW 66
struct DxArgs {
    const float *W, *dEdXt, *Yt_prev;
    float *dEdXt_prev, *dEdX_prev;
    int Kp, Np, Bp, k_tiles, b_tiles, map, b_shift;
};
// per wave: W piece [32][66] + dEdXt piece [64][32]; LDS-DMA form (PIPE 4): two sets of two unpadded 8 KB tiles.
// Two forms are left, both 4 waves with the main loop pipelined inside the wave: operands by LDS-DMA (PIPE 4) or through
// staging registers (PIPE 1); the host picks one from the shape (engine.hip dx_dma).  The parameter lists are kept as
// they were, so that the kernels keep their names.
template <int NW, int PIPE> constexpr int dx_lds_floats() {
    static_assert(NW == 4 && (PIPE == 4 || PIPE == 1), "the dX kernels have two forms");
    return NW * (PIPE == 4 ? 8192 : 32 * DX_LDW + 2048) + 32 * 36;
}

template <int NW, int PIPE = 1, int ACT = ACT_SIGMOID>
__device__ __forceinline__ void dx_body(const DxArgs &A, const int bid, float *smem, long long *stamps) {
    static_assert(NW == 4 && (PIPE == 4 || PIPE == 1), "the dX kernels have two forms");
    const float *__restrict__ W = A.W, *__restrict__ dEdXt = A.dEdXt, *__restrict__ Yt_prev = A.Yt_prev;
    float *__restrict__ dEdXt_prev = A.dEdXt_prev, *__restrict__ dEdX_prev = A.dEdX_prev;
    const int Kp = A.Kp, Np = A.Np, Bp = A.Bp, k_tiles = A.k_tiles, b_tiles = A.b_tiles;
    // per wave: W piece [32][66] (2112 floats) + dEdXt piece [64 n][32] (2048 floats)
    constexpr int WSZ = 32 * DX_LDW, STG = PIPE == 4 ? 8192 : WSZ + 2048;
    float(*tileT)[36] = reinterpret_cast<float(*)[36]>(smem + NW * STG);
    stamp(stamps, 0, bid);
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int i = lane & 31, h = lane >> 5;
    int kt, bt;
    tile_of_block(bid, k_tiles, b_tiles, A.b_shift, kt, bt, A.map);
    const int k0 = kt * 32, b0 = bt * 32;

    const int Q = Np >> 2;             // quads of 4 consecutive n
    const int qw = (Q + NW - 1) / NW;  // quads per wave (the last waves may run short or empty)
    const int q0 = wave * qw;
    const int qend = (q0 + qw < Q) ? q0 + qw : Q;
    const int myq = qend > q0 ? qend - q0 : 0;
    const int nch = (myq + 15) >> 4;   // chunks of 16 quads = 64 n

    float *wb = smem + wave * STG, *db = wb + WSZ;
    const rsrc_t rW = make_rsrc(W, (size_t)Kp * Np * 4), rD = make_rsrc(dEdXt, (size_t)Np * Bp * 4);
    const int wc4 = lane & 15, wr0 = lane >> 4;  // W staging: 16 lanes per row, 4 rows per instruction
    const int voW = ((k0 + wr0) * Np + 4 * wc4) * 4;
    const int r8 = lane >> 3, c4 = lane & 7;      // dEdXt staging: 8 lanes per row, 8 rows per instruction
    const int voD = (r8 * Bp + b0 + 4 * c4) * 4;
    // Columns 32..63 of a W-piece row are stored with their dword PAIRS swapped (n -> n ^ 2): the two 8-byte stores
    // of a lane's float4 then go to dwords {4c, 4c+1} / {4c+2, 4c+3} for c < 8 and to {4c+2, 4c+3} / {4c, 4c+1} for
    // c >= 8, so the 16 lanes of one ds_write_b64 group (one row) cover all 32 banks once.  Written in natural
    // order, lanes c and c+8 hit the same bank pair: the 2-way conflict SQ_LDS_BANK_CONFLICT showed for this
    // kernel in round 1 (192 cycles per wave, 20 % of its LDS cycles).  The reads below undo the swap.
    const int wsw = (wc4 >= 8) ? 2 : 0;
    float *wdst = wb + wr0 * DX_LDW + 4 * wc4;
    // rows of the dEdXt piece are stored with bits 0 and 1 of the row number swapped: the two half-waves of a
    // fragment read (rows 4j and 4j+2, or 4j+1 and 4j+3) then sit 32 words apart, in different bank halves,
    // and the two values a lane needs per MFMA pair sit 64 words apart: one ds_read2st64_b32 (-0.8 us)
    float *ddst = db + ((r8 & ~3) | ((r8 & 1) << 1) | ((r8 >> 1) & 1)) * 32 + 4 * c4;
    const float *ard = wb + i * DX_LDW + 2 * h;            // n < 32: natural order
    const float *ard_hi = wb + i * DX_LDW + 2 * (1 - h);   // n >= 32: dword pairs swapped (see wsw)
    const float *brd = db + h * 32 + i;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;

    // the epilogue's global operand (y of this thread's output elements, for the sigmoid derivative) is fetched now,
    // above a compiler-level fence, not behind the last barrier (see fwd_body)
    float4 y_pre4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // a thread owns 4 consecutive frames of one unit
    if constexpr (ACT == ACT_VIS_LINEAR || ACT == ACT_VIS_SIGMOID) {
        y_pre4.x = Yt_prev[k0 + (tid >> 3)];  // the visible bias c [Kp] of this thread's unit (rbm.hip.h)
    } else {
        y_pre4 = *reinterpret_cast<const float4 *>(&Yt_prev[(size_t)(k0 + (tid >> 3)) * Bp + b0 + (tid & 7) * 4]);
    }
    asm volatile("" ::: "memory");

    if constexpr (PIPE == 4) {
    // LDS-DMA form (see fwd_body): both pieces of a chunk go global -> LDS directly, into one of two tile sets.
    // The dEdXt piece keeps its layout (a wave-load = 8 rows of 128 B; the row permutation moves into the per-lane
    // global offset).  The W piece cannot keep the 66-float row stride -- a DMA writes lane-linear 16-byte slots --
    // so its [32 k][16 quads] slots are filled with quad (q ^ (k & 15)) of row k: the global reads stay whole
    // 256-byte row segments, and the 32 lanes of a transposed fragment read (one per row k, same quad) spread over
    // the 16 slot columns instead of hitting one (a 2-way conflict is left: 16-byte slots, 8-byte reads).
    float *ws0 = smem + wave * STG, *ds0 = ws0 + 2048, *ws1 = ws0 + 4096, *ds1 = ws0 + 6144;
    const int endW = Kp * Np * 4, endD = Np * Bp * 4;
    const int wr = lane >> 4, wq = lane & 15;  // W DMA: 4 rows x 16 slots per instruction
    int voWd[4];
#pragma unroll
    for (int tt = 0; tt < 4; tt++) voWd[tt] = ((k0 + wr) * Np + 4 * (wq ^ (4 * tt + wr))) * 4;
    const int voDd = (((r8 & ~3) | ((r8 & 1) << 1) | ((r8 >> 1) & 1)) * Bp + b0 + 4 * c4) * 4;
    int aoff[16];  // fragment read offsets (floats) of this lane's row: quad j sits in slot j ^ (i & 15)
#pragma unroll
    for (int j = 0; j < 16; j++) aoff[j] = i * 64 + 4 * (j ^ (i & 15)) + 2 * h;
    const int boff = h * 32 + i;
    float fa[32], fb[32], ga[32], gb[32];
#define DX_DMA1(WS, DS, C, T)                                                              \
    {                                                                                      \
        const int quad0 = q0 + (C)*16;                                                     \
        const bool live = (C) < nch;                                                       \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (__attribute__((address_space(3))) void *)(WS + (T) * 256), 16, \
                                                 voWd[(T) & 3], live ? quad0 * 16 + (T) * (16 * Np) : endW, 0, 0); \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rD, (__attribute__((address_space(3))) void *)(DS + (T) * 256), 16, \
                                                 voDd, live ? (4 * quad0 + 8 * (T)) * Bp * 4 : endD, 0, 0); \
    }
#define DX_RD1(WS, DS, NA, NB, J)                                                          \
    {                                                                                      \
        NA[2 * (J)] = (WS)[aoff[J]];                                                       \
        NA[2 * (J) + 1] = (WS)[aoff[J] + 1];                                               \
        NB[2 * (J)] = (DS)[boff + (4 * (J)) * 32];                                         \
        NB[2 * (J) + 1] = (DS)[boff + (4 * (J) + 2) * 32];                                 \
    }
    // chunk C on (FA, FB), read from set (WC, DC) one body ago; chunk C+1 is in / landing in set (WN, DN); C+2 -> (WC, DC)
#define DX_BODYD(FA, FB, NA, NB, WC, DC, WN, DN, C)                                        \
    {                                                                                      \
        __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0): the fragment reads of (WC, DC) have returned */ \
        _Pragma("unroll") for (int g = 0; g < 8; g++) {                                    \
            acc = mfma32(FA[2 * g], FB[2 * g], acc);                                       \
            acc = mfma32(FA[2 * g + 1], FB[2 * g + 1], acc);                               \
            DX_DMA1(WC, DC, (C) + 2, g);                                                   \
            __builtin_amdgcn_sched_barrier(0);                                             \
        }                                                                                  \
        __builtin_amdgcn_s_waitcnt(0x4F70); /* vmcnt(16): chunk C+1 has landed, the 16 loads of C+2 may be in flight */ \
        _Pragma("unroll") for (int g = 8; g < 16; g++) {                                   \
            acc = mfma32(FA[2 * g], FB[2 * g], acc);                                       \
            acc = mfma32(FA[2 * g + 1], FB[2 * g + 1], acc);                               \
            DX_RD1(WN, DN, NA, NB, 2 * (g - 8));                                           \
            DX_RD1(WN, DN, NA, NB, 2 * (g - 8) + 1);                                       \
            __builtin_amdgcn_sched_barrier(0);                                             \
        }                                                                                  \
    }
#define DX_DRAIND(FA, FB, CNT)                                                             \
    {                                                                                      \
        _Pragma("unroll") for (int j = 0; j < 16; j++) {                                   \
            if (j < (CNT)) {                                                               \
                acc = mfma32(FA[2 * j], FB[2 * j], acc);                                   \
                acc = mfma32(FA[2 * j + 1], FB[2 * j + 1], acc);                           \
            }                                                                              \
        }                                                                                  \
    }
    if (nch > 0) {
        const int nfull = myq >> 4, rem = myq & 15;
#pragma unroll
        for (int t = 0; t < 8; t++) DX_DMA1(ws0, ds0, 0, t);
#pragma unroll
        for (int t = 0; t < 8; t++) DX_DMA1(ws1, ds1, 1, t);
        __builtin_amdgcn_s_waitcnt(0x4F70);  // vmcnt(16)
#pragma unroll
        for (int j = 0; j < 16; j++) DX_RD1(ws0, ds0, fa, fb, j);
        __builtin_amdgcn_sched_barrier(0);
        int c = 0;
        for (; c + 1 < nfull; c += 2) {
            DX_BODYD(fa, fb, ga, gb, ws0, ds0, ws1, ds1, c);
            DX_BODYD(ga, gb, fa, fb, ws1, ds1, ws0, ds0, c + 1);
        }
        if (c < nfull) {
            DX_BODYD(fa, fb, ga, gb, ws0, ds0, ws1, ds1, c);
            DX_DRAIND(ga, gb, rem);
        } else {
            DX_DRAIND(fa, fb, rem);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): nothing may still be landing when the reduction reuses the LDS
    }
#undef DX_DMA1
#undef DX_RD1
#undef DX_BODYD
#undef DX_DRAIND
    } else {
    // Software-pipelined inside the wave like fwd_body's loop: the 32 MFMAs of chunk c (16 quads = 64 n) run on
    // fragments already in registers; in their shadow chunk c+1 goes registers -> LDS (groups 0..7) -> fragments
    // (groups 8..15) and the staging registers are refilled with chunk c+2 four groups after they were stored
    // (1.5 us of lead at two waves per SIMD).  One staging set instead of two pays for the second fragment set.
    // Same MFMA order as the round-1 loop: same bits.
    float4 wa[8], da[8];
    float fa[32], fb[32], ga[32], gb[32];
    // chunks past this wave's last one: from the end of the buffer = zeros without a memory request (see fwd_body)
    const int endW = Kp * Np * 4, endD = Np * Bp * 4;
#define DX_LOAD1(C, IT)                                                                    \
    {                                                                                      \
        const int quad0 = q0 + (C)*16;                                                     \
        const bool live = (C) < nch;                                                       \
        wa[IT] = bload4(rW, voW, live ? quad0 * 16 + (IT) * (16 * Np) : endW);             \
        da[IT] = bload4(rD, voD, live ? (4 * quad0 + 8 * (IT)) * Bp * 4 : endD);           \
    }
#define DX_WRITE1(IT)                                                                      \
    {                                                                                      \
        float *dst = wdst + (4 * (IT)) * DX_LDW;                                           \
        *reinterpret_cast<float2 *>(dst + wsw) = make_float2(wa[IT].x, wa[IT].y);          \
        *reinterpret_cast<float2 *>(dst + (2 - wsw)) = make_float2(wa[IT].z, wa[IT].w);    \
        *reinterpret_cast<float4 *>(ddst + (IT) * 256) = da[IT];                           \
    }
#define DX_READ1(NA, NB, J)                                                                \
    {                                                                                      \
        const float2 av = *reinterpret_cast<const float2 *>(((J) < 8 ? ard : ard_hi) + 4 * (J)); \
        NA[2 * (J)] = av.x;                                                                \
        NA[2 * (J) + 1] = av.y;                                                            \
        NB[2 * (J)] = brd[(4 * (J)) * 32];                                                 \
        NB[2 * (J) + 1] = brd[(4 * (J) + 2) * 32];                                         \
    }
#define DX_BODY(FA, FB, NA, NB, C)                                                         \
    {                                                                                      \
        _Pragma("unroll") for (int g = 0; g < 16; g++) {                                   \
            acc = mfma32(FA[2 * g], FB[2 * g], acc);                                       \
            acc = mfma32(FA[2 * g + 1], FB[2 * g + 1], acc);                               \
            if (g < 8) DX_WRITE1(g);                                                       \
            if (g >= 4 && g < 12) DX_LOAD1((C) + 2, g - 4);                                \
            if (g >= 8) {                                                                  \
                DX_READ1(NA, NB, 2 * (g - 8));                                             \
                DX_READ1(NA, NB, 2 * (g - 8) + 1);                                         \
            }                                                                              \
            __builtin_amdgcn_sched_barrier(0);                                             \
        }                                                                                  \
    }
#define DX_DRAIN(FA, FB, CNT)                                                              \
    {                                                                                      \
        _Pragma("unroll") for (int j = 0; j < 16; j++) {                                   \
            if (j < (CNT)) {                                                               \
                acc = mfma32(FA[2 * j], FB[2 * j], acc);                                   \
                acc = mfma32(FA[2 * j + 1], FB[2 * j + 1], acc);                           \
            }                                                                              \
        }                                                                                  \
    }
    if (nch > 0) {
        const int nfull = myq >> 4, rem = myq & 15;
#pragma unroll
        for (int it = 0; it < 8; it++) DX_LOAD1(0, it);
#pragma unroll
        for (int it = 0; it < 8; it++) DX_WRITE1(it);
#pragma unroll
        for (int j = 0; j < 16; j++) DX_READ1(fa, fb, j);
#pragma unroll
        for (int it = 0; it < 8; it++) DX_LOAD1(1, it);
        __builtin_amdgcn_sched_barrier(0);
        int c = 0;
        for (; c + 1 < nfull; c += 2) {
            DX_BODY(fa, fb, ga, gb, c);
            DX_BODY(ga, gb, fa, fb, c + 1);
        }
        if (c < nfull) {
            DX_BODY(fa, fb, ga, gb, c);
            DX_DRAIN(ga, gb, rem);
        } else {
            DX_DRAIN(fa, fb, rem);
        }
    }
#undef DX_LOAD1
#undef DX_WRITE1
#undef DX_READ1
#undef DX_BODY
#undef DX_DRAIN
    }

    stamp(stamps, 1, bid);
    __syncthreads();
    float(*red)[1024] = reinterpret_cast<float(*)[1024]>(smem);
#pragma unroll
    for (int r = 0; r < 16; r++) red[wave][acc_row(r, lane) * 32 + i] = acc[r];
    __syncthreads();
    stamp(stamps, 2, bid);
    // see fwd_body: ds_read_b128 of the partial tiles, 16-byte stores of both layouts
    const int row = tid >> 3, col4 = (tid & 7) * 4;
    float4 d4 = *reinterpret_cast<const float4 *>(&red[0][row * 32 + col4]);
#pragma unroll
    for (int w = 1; w < NW; w++) {
        const float4 p4 = *reinterpret_cast<const float4 *>(&red[w][row * 32 + col4]);
        d4.x += p4.x;
        d4.y += p4.y;
        d4.z += p4.z;
        d4.w += p4.w;
    }
    float4 g4;  // kernDsigmoid, DevFunc.cu:67-68
    if constexpr (ACT == ACT_VIS_LINEAR) {  // an RBM's reconstruction (rbm_rule.h): v1 = h0s W^T + c
        g4.x = d4.x + y_pre4.x;
        g4.y = d4.y + y_pre4.x;
        g4.z = d4.z + y_pre4.x;
        g4.w = d4.w + y_pre4.x;
    } else if constexpr (ACT == ACT_VIS_SIGMOID) {  // ... and sigma of it for Bernoulli visibles
        g4.x = sigmoid_det(d4.x + y_pre4.x);
        g4.y = sigmoid_det(d4.y + y_pre4.x);
        g4.z = sigmoid_det(d4.z + y_pre4.x);
        g4.w = sigmoid_det(d4.w + y_pre4.x);
    } else if constexpr (ACT == ACT_RELU) {
        g4.x = drelu(y_pre4.x, d4.x);
        g4.y = drelu(y_pre4.y, d4.y);
        g4.z = drelu(y_pre4.z, d4.z);
        g4.w = drelu(y_pre4.w, d4.w);
    } else {
        g4.x = (1.0f - y_pre4.x) * y_pre4.x * d4.x;
        g4.y = (1.0f - y_pre4.y) * y_pre4.y * d4.y;
        g4.z = (1.0f - y_pre4.z) * y_pre4.z * d4.z;
        g4.w = (1.0f - y_pre4.w) * y_pre4.w * d4.w;
    }
    *reinterpret_cast<float4 *>(&dEdXt_prev[(size_t)(k0 + row) * Bp + b0 + col4]) = g4;
    tileT[col4][row] = g4.x;
    tileT[col4 + 1][row] = g4.y;
    tileT[col4 + 2][row] = g4.z;
    tileT[col4 + 3][row] = g4.w;
    __syncthreads();
    *reinterpret_cast<float4 *>(&dEdX_prev[(size_t)(b0 + row) * Kp + k0 + col4]) =
        *reinterpret_cast<const float4 *>(&tileT[row][col4]);
    stamp(stamps, 3, bid);
}

// ---------------------------------------------------------------------------------------
// Weight-gradient GEMM with the SGD update as its epilogue:
//   G[k][n] = sum_b Y[b][k] * dEdX[b][n]
//   delta = mom*delta - lr*(G/n_frames + wc*W) ;  W = delta + 1.0f*W
// replaces cublasSgemm(N,T) + kernUpdatedelta + kernAccSum (BP_GPU.cu:432-436,
// DevFunc.cu:490-507,427-443): one pass over W/delta instead of seven.  This kernel is
// HBM-bound (16 bytes of W/delta traffic per 2*B flops), so it is built around the memory
// system:
//  * workgroup tile 64T x 64T (T=2: 128x128), 4 waves as 2x2, wave tile 32T x 32T;
//  * both operand tiles ([<=128 frames][64T] of Y and of dEdX, row-major) are staged ONCE
//    into LDS with coalesced 16-byte loads (<= 128 KB, one workgroup per CU);
//  * the W and delta tiles are prefetched into registers (coalesced 16-byte loads, 4 rows x
//    16T floats per wave-instruction) right after staging, so they stream from HBM while the
//    MFMA loop -- which then issues no vector-memory instruction at all -- runs from LDS;
//  * the accumulators are transposed through LDS (operand space is dead by then) into the
//    same row-contiguous float4 layout, updated and stored with coalesced 16-byte stores.
// Column assignment: MFMA tile t of a wave covers columns T*i + t (i = lane&31), so one
// ds_read_b{32T} per operand feeds all T tiles.
// FUSED=false writes G instead (data-parallel path: all-reduced before k_apply_update).
// Rows k >= K are skipped (layer 1 reads the caller's unpadded chunk, whose columns past K
// alias the next frame); columns n >= N need no mask because dEdX pads are exact zeros.
// ---------------------------------------------------------------------------------------
template <int T> struct VecT;
template <> struct VecT<1> { typedef float type; };
template <> struct VecT<2> { typedef float2 type; };
__device__ __forceinline__ float vget(float v, int) { return v; }
__device__ __forceinline__ float vget(float2 v, int t) { return t == 0 ? v.x : v.y; }

template <int T, bool FUSED>
__global__ __launch_bounds__(256) void k_dw(const float *__restrict__ Yrow, int ldA, const float *__restrict__ dEdX,
                                            float *__restrict__ Wt, float *__restrict__ delta,
                                            float *__restrict__ G, float *__restrict__ bias,
                                            float *__restrict__ dbias, float *__restrict__ gb, int K, int N, int Np,
                                            int B, int Bp, int n_wg, float nf, float mom, float lr, float wc,
                                            long long *stamps) {
    stamp(stamps, 0);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int TW = 64 * T;      // workgroup tile width (both dims)
    constexpr int WT = 32 * T;      // wave tile width
    constexpr int QPR = WT / 4;     // float4 per wave-tile row
    constexpr int RPP = 64 / QPR;   // wave-tile rows per epilogue pass
    constexpr int NPASS = WT / RPP; // epilogue passes (4*T*T)
    constexpr int SQ = TW / 4;      // float4 per staged row
    constexpr int SRP = 256 / SQ;   // staged rows per pass
    constexpr int CH = 64 * T;      // frames staged per pass (LDS = 2*CH*TW floats: 32 KB / 128 KB)
    float *As = lds, *Bs = lds + CH * TW;
    typedef typename VecT<T>::type vec_t;

    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int i = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int kt = blockIdx.x / n_wg, ntile = blockIdx.x % n_wg;
    const int k0 = kt * TW, n0 = ntile * TW;

    const rsrc_t rA = make_rsrc(Yrow, (size_t)Bp * ldA * 4), rB = make_rsrc(dEdX, (size_t)Bp * Np * 4);

    f32x16 acc[T][T];
#pragma unroll
    for (int tm = 0; tm < T; tm++)
#pragma unroll
        for (int tn = 0; tn < T; tn++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[tm][tn][r] = 0.0f;

    // epilogue geometry (also the prefetch geometry)
    const int ec = lane % QPR, er = lane / QPR;
    const int gk0 = k0 + WT * wm + er, gn = n0 + WT * wn + 4 * ec;
    float4 wreg[NPASS], dreg[NPASS];

    const int scol = tid % SQ, srow = tid / SQ;
    float bsum = 0.0f;  // bias gradient of column n0+tid (first k-tile row of workgroups only)
    for (int bc = 0; bc < Bp; bc += CH) {
        const int rows = (Bp - bc < CH) ? (Bp - bc) : CH;
        // ---- stage both operand tiles, 8 float4 per operand per batch
        for (int r0 = 0; r0 < rows; r0 += 8 * SRP) {
            float4 sa[8], sb[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int row = r0 + srow + q * SRP;
                sa[q] = bload4(rA, ((bc + row) * ldA + k0 + 4 * scol) * 4, 0);
                sb[q] = bload4(rB, ((bc + row) * Np + n0 + 4 * scol) * 4, 0);
            }
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int row = r0 + srow + q * SRP;
                if (row < rows) {
                    *reinterpret_cast<float4 *>(As + row * TW + 4 * scol) = sa[q];
                    *reinterpret_cast<float4 *>(Bs + row * TW + 4 * scol) = sb[q];
                }
            }
        }
        __syncthreads();
        if (bc == 0) stamp(stamps, 1);
        if (kt == 0 && tid < TW) {
            // bias gradient: frames summed sequentially in fp32 (kernAccSumrow order,
            // DevFunc.cu:267-285 <- BP_GPU.cu:434); the dEdX tile is in LDS anyway
            const float *col = Bs + tid;
            int b = 0;
            const int bend = (B - bc < rows) ? (B - bc) : rows;
            if (bc == 0 && bend > 0) {
                bsum = col[0];
                b = 1;
            }
            for (; b + 16 <= bend; b += 16) {
                float v[16];
#pragma unroll
                for (int u = 0; u < 16; u++) v[u] = col[(b + u) * TW];
#pragma unroll
                for (int u = 0; u < 16; u++) bsum += v[u];
            }
            for (; b < bend; b++) bsum += col[b * TW];
        }
        if (FUSED && bc == 0) {
            // W / delta prefetch: in flight during the whole MFMA loop
#pragma unroll
            for (int it = 0; it < NPASS; it++) {
                const int k = gk0 + RPP * it;
                if (k < K && gn < Np) {
                    const size_t idx = (size_t)k * Np + gn;
                    wreg[it] = *reinterpret_cast<const float4 *>(Wt + idx);
                    dreg[it] = *reinterpret_cast<const float4 *>(delta + idx);
                } else {
                    wreg[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                    dreg[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        }
        if (bc == 0) stamp(stamps, 2);
        // ---- MFMA loop over frame pairs, operands from LDS only
        const float *ap = As + h * TW + WT * wm + T * i;
        const float *bp = Bs + h * TW + WT * wn + T * i;
        for (int p0 = 0; p0 < rows / 2; p0 += 8) {  // rows % 32 == 0
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const vec_t a = *reinterpret_cast<const vec_t *>(ap + 2 * (p0 + u) * TW);
                const vec_t b = *reinterpret_cast<const vec_t *>(bp + 2 * (p0 + u) * TW);
#pragma unroll
                for (int tm = 0; tm < T; tm++)
#pragma unroll
                    for (int tn = 0; tn < T; tn++) acc[tm][tn] = mfma32(vget(a, tm), vget(b, tn), acc[tm][tn]);
            }
        }
        __syncthreads();
    }

    stamp(stamps, 3);
    if (kt == 0 && tid < TW) {
        const int n = n0 + tid;
        if (n < N) {
            if (FUSED) {  // kernUpdatedelta with weightcost 0 + kernAccSum, BP_GPU.cu:435,437
                const float bv = bias[n];
                const float d = mom * dbias[n] - lr * (bsum / nf + 0.0f * bv);
                dbias[n] = d;
                bias[n] = d + 1.0f * bv;
            } else {
                gb[n] = bsum;
            }
        }
    }
    // ---- epilogue: accumulators -> LDS (wave-private [WT][WT] tile) -> row-contiguous float4
    float *Tw = lds + wave * (WT * WT);
#pragma unroll
    for (int tm = 0; tm < T; tm++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int kl = T * acc_row(r, lane) + tm;
            if (T == 2) {
                *reinterpret_cast<float2 *>(Tw + kl * WT + 2 * i) = make_float2(acc[tm][0][r], acc[tm][T - 1][r]);
            } else {
                Tw[kl * WT + i] = acc[tm][0][r];
            }
        }
    __syncthreads();
    stamp(stamps, 4);
#pragma unroll
    for (int it = 0; it < NPASS; it++) {
        const int kl = er + RPP * it;
        const int k = gk0 + RPP * it;
        const float4 g = *reinterpret_cast<const float4 *>(Tw + kl * WT + 4 * ec);
        if (k < K && gn < Np) {
            const size_t idx = (size_t)k * Np + gn;
            if (FUSED) {
                const float4 w = wreg[it];
                float4 d = dreg[it];
                // kernUpdatedelta (DevFunc.cu:502) then kernAccSum (DevFunc.cu:440)
                d.x = mom * d.x - lr * (g.x / nf + wc * w.x);
                d.y = mom * d.y - lr * (g.y / nf + wc * w.y);
                d.z = mom * d.z - lr * (g.z / nf + wc * w.z);
                d.w = mom * d.w - lr * (g.w / nf + wc * w.w);
                *reinterpret_cast<float4 *>(delta + idx) = d;
                *reinterpret_cast<float4 *>(Wt + idx) =
                    make_float4(d.x + 1.0f * w.x, d.y + 1.0f * w.y, d.z + 1.0f * w.z, d.w + 1.0f * w.w);
            } else {
                *reinterpret_cast<float4 *>(G + idx) = g;
            }
        }
    }
    stamp(stamps, 5);
}

// ---------------------------------------------------------------------------------------
// Persistent, software-pipelined form of k_dw (same math, same outputs) for Bp = 64*H:
// 64x64 tiles, <= 2 workgroups per CU, each walking tiles t = blockIdx.x, += gridDim.x.
// A "unit" is one 64-frame slice of a tile's two operand tiles (32 KB of LDS, two buffers).
// While unit u runs on the MFMA pipe, the 16-byte loads of unit u+1 (straight into the other LDS
// buffer, by LDS-DMA) and 1/H of the NEXT tile's W/delta tiles (to one of two register sets) are in
// flight, so memory streams continuously instead of in per-workgroup bursts (the stage -> MFMA ->
// store lock-step of k_dw).
// What bounds it (profiles/r01_sq_counters.txt, r01_vmem_rate.txt): its memory-
// pipeline time (118 MB of stores at 27 ns per dwordx4 store and CU, 351 MB of loads at 7 ns) and its
// MFMA time add up instead of overlapping; the per-unit loads are therefore interleaved with the
// MFMAs in the instruction stream (the groups of DWP_UNIT), the only placement that overlaps on this
// chip (tools/overlap_probe.hip).  Every global access is an UNCONDITIONAL buffer
// load/store whose out-of-range cases (pad rows k >= K, no next tile) are expressed through the
// offset / an empty descriptor and dropped by the hardware range check: with no branch
// around any memory instruction the s_waitcnt vmcnt(N) before a unit's hand-off barrier
// leaves exactly the younger stores and W/delta prefetch loads in flight.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void bstore1(float v, rsrc_t r, int voff) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, 0, 0);
}
__device__ __forceinline__ void bstore4(float4 v, rsrc_t r, int voff) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), r, voff, 0, 0);
}

// One layer's share of a launch, as the host describes it (engine.hip dwp_args); the kernel walks the tile records
// made of it (DwpDesc below).  Hyper-parameters and the frame count travel in DwpConst.
struct DwpArgs {
    const float *Yrow, *dEdX;
    float *Wt, *delta, *G, *bias, *dbias, *gb;
    int ldA, K, N, Kp, Np, n_wg, ntiles;
    // sharded data parallel: the job covers tile rows k_first .. of the layer;
    // wd_off = 1 makes it a bias-only job (W/delta are neither read nor written: the tiles of weight
    // row block 0 run on every rank so that every rank applies the same bias update); do_bias = 0
    // suppresses the bias update of a job that does own row block 0
    int k_first, wd_off, do_bias;
    int k_base;  // first unit that Yrow's columns hold (0: all of them; all-to-all form: the rank's block starts here)
    int pad_;    // always 0: no padding bytes, so two job lists are equal exactly when their bytes are (engine.hip dwp_table)
};
// One launch may walk the tiles of several layers (every dW(l) only needs dEdX_l and Y_{l-1}, both
// final once the last dX has run): job j owns the global tile numbers [tile_end[j-1], tile_end[j]).
constexpr int DWP_MAXJOBS = 20;
struct DwpJobs {
    DwpArgs job[DWP_MAXJOBS];
    int tile_end[DWP_MAXJOBS];
    int njobs, total;
};
constexpr int dwp_lds_floats() { return 2 * 8192; }

// Everything the pipeline needs to know about one 64x64 tile, as ONE 64-byte record of a table the host builds
// once per launch plan (engine.hip dwp_table): the walk t -> (layer, k0, n0, pointers) used to be done by every wave
// at the start of every tile -- a scan of the job table in kernel-argument memory, an integer division and two
// more dependent scalar loads, ~1.5k cycles during which the wave issued no MFMA (tools/dwp_phases.py, round 2).
// Now it is one 64-byte record fetched a whole tile ahead: ONE vector load per wave (lanes 0..3 take a quarter
// each), turned into scalars with v_readlane when the tile becomes current.  (A scalar load would be the obvious
// instruction, but SMEM shares the lgkmcnt counter with LDS and returns out of order, so every LDS fragment read
// issued while it is in flight has to be waited for with lgkmcnt(0) -- the record's memory latency then lands in
// front of the tile's first MFMA.)  All pointers are already offset to the tile.
struct DwpDesc {
    const float *A;   // Y_{l-1} + k0            (rows = frames, row stride ldA)
    const float *Bm;  // dEdX_l + n0             (row stride Np)
    float *W;         // FUSED: W_l + k0*Np + n0;      otherwise G_l + k0*Np + n0
    float *D;         // FUSED: delta_l + k0*Np + n0
    float *bias;      // tiles of weight-row block 0 that own the bias update: FUSED bias_l + n0, otherwise gb_l + n0
    float *dbias;     // FUSED: dbias_l + n0
    int ldA, Np;
    unsigned packed;  // rows | colsw << 8 | nbias << 16 | valid << 24: weight rows / columns of the tile that exist
                      // (0 rows: bias-only tile, W / delta are not touched), bias columns this tile updates (0: none)
    unsigned szW;     // bytes from W (and D) to the end of the tile's last real row (at most to the end of the layer's
                      // matrix): the range the stores may touch -- the descriptor's range check IS the row test
};
static_assert(sizeof(DwpDesc) == 64, "four 16-byte quarters per record");
struct DwpRaw {
    unsigned w[16];
};
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// the quarter this lane fetched (lanes 0..3 hold the whole record) -> wave-uniform record
__device__ __forceinline__ DwpDesc dwp_decode(u32x4 v) {
    DwpRaw r;
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int c = 0; c < 4; c++) r.w[4 * q + c] = (unsigned)__builtin_amdgcn_readlane((int)v[c], q);
    return __builtin_bit_cast(DwpDesc, r);
}
struct DwpConst {
    int B;  // frames of the (global) minibatch: the bias gradient sums rows 0..B-1
    float nf, mom, lr, wc;
};

// bid / nblocks: this workgroup's index and the number of workgroups walking the tiles; the table holds
// total + 2*nblocks records (the tail ones invalid: their loads return zeros, their stores are dropped).
//
// Schedule (round 2; tools/dwp_phases.py showed a wave spending only half of a tile's cycles issuing MFMAs: the
// rest was the tile walk, the epilogue and the operand hand-offs, during which its SIMD's matrix pipe had at
// best the other workgroup's wave to run).  Now the wave's MFMA stream never stops for the epilogue:
//   * the epilogue of tile t (accumulators -> LDS transposition -> momentum / weight-decay update -> 8 stores)
//     is issued BETWEEN the MFMAs of the first unit of tile t+1, on a second accumulator set (the compiler renames
//     the 16 accumulator registers; nothing is copied);
//   * the W / delta tiles of tile t+1 are loaded during the LAST unit of tile t (between its MFMAs) and consumed a
//     whole tile later, in the first unit of tile t+2: under load an HBM read takes longer than one unit lasts (a
//     version that loaded them one unit ahead stalled ~2k cycles per tile on them), hence two register sets, used
//     alternately: tile t's pending epilogue frees the set that the same tile's last unit refills;
//   * every unit is ONE basic block whose issue order is written out group by group -- {2 MFMAs, the LDS fragment
//     reads of the pair after next, one or two memory / epilogue operations} x 16 -- with a scheduling fence
//     after each group: MFMA and memory work only overlap when interleaved in ONE wave's stream
//     (profiles/r01_overlap_probe.txt), and an MFMA never waits for an LDS read issued just before it;
//   * the transposition scratch of wave w lives in the 16 rows of the buffer being refilled that only wave w
//     writes (rows 4w..4w+3 of every group of 16), used before the wave's own operand writes: no barrier;
//   * the bias gradient / update of the tiles of weight-row block 0 stays outside the blocks (divergent, rare).
// POW2: the minibatch size is a power of two, so G / n == G * (1/n) bit for bit (also when the result is subnormal:
// both are the correctly rounded value of the same real number) and the ~10-instruction IEEE division per weight is
// a multiply; chosen by the host (a run-time branch would split the blocks).
// PHASES: diagnostic twin only (mlggd_debug_stamp_select("dw", -1)): wave 0 sums the shader-clock cycles of
// [0] units 0..H-2 up to the last MFMA issue, [1] their hand-off (vmcnt wait, LDS write, barrier), [2] the last
// unit, [3] unused, [4] the last hand-off, over all its tiles -> row nblocks + bid of the stamp buffer.
// BIAS_ONLY: the tiles of k_dwp_bias (no weight rows: only the operand staging and the bias gradient / update are
// needed): compiles out the fragment reads, the MFMAs, the pending epilogue's update and stores inside the unit
// blocks, and the W / delta loads of the next tile.
template <int H, bool FUSED, bool POW2, bool PHASES = false, bool BIAS_ONLY = false>
__device__ __forceinline__ void dwp_body(const DwpDesc *__restrict__ table, const int total, const DwpConst C, const int bid,
                                         const int nblocks, float *lds, long long *stamps) {
    stamp_clk(stamps, 0, bid);  // diagnostic (nullptr in every normal launch): wall + shader clock at start / end
    const int B = C.B;
    const float nf = C.nf, mom = C.mom, lr = C.lr, wc = C.wc;
    const float inv_nf = 1.0f / nf;
    constexpr unsigned OOB = 0x7F000000u;  // byte offset beyond every descriptor: load -> 0, store dropped
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int i = lane & 31, h5 = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int scol = tid & 15, srow = tid >> 4;  // staging: 16 float4 per 64-float row, 16 rows per pass
    const int ec = lane & 7, er = lane >> 3;     // epilogue: 8 float4 per 32-float wave-tile row

    f32x16 acc, accp;  // this tile's accumulators; the previous tile's, whose epilogue is pending
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = accp[r] = 0.0f;
    // the first unit's operands on their way global -> LDS: only the prologue uses these and DWP_WRITE_UNIT, but
    // declared inside the prologue's block they reorder the instructions of every FUSED kernel
    float4 ra[4], rb[4];
    // W / delta of tiles k (set k & 1): set 1 is consumed by the (empty) pending epilogue of the first tile
    float4 pw0[4], pd0[4], pw1[4], pd1[4];
#pragma unroll
    for (int q = 0; q < 4; q++) pw1[q] = pd1[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    float bsum = 0.0f, bsum_p = 0.0f;

    // (no early return for bid >= total: the host never launches more workgroups than tiles, and the test would sit
    // between the kernel's argument loads -- fetch `total`, wait, branch, only then fetch the rest.  Such a workgroup
    // would walk one tile of invalid records: every load returns zeros, every store is dropped.)
    int t = bid;
    const rsrc_t rT = make_rsrc(table, ((size_t)total + 2 * (size_t)nblocks) * sizeof(DwpDesc));
    const int voT = 16 * (lane & 3);
#define DWP_FETCH(TI) __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rT, voT, (TI) * 64, 0))
    // current tile, next tile (its record for the one after is in flight during the whole current tile), and the
    // previous one, whose epilogue is pending: at first an invalid record (no rows: every store is dropped)
    // The bias pointers of a record (its third quarter) are not decoded with the rest: three live records of 16
    // scalars each beside six resource descriptors do not fit the scalar file, and the compiler spilled them into
    // VGPR lanes inside the tile loop.  They stay in the fetched vector (4 VGPRs per record, of which there are
    // plenty) and become scalars only inside the rare, divergent bias update.
    u32x4 tc_raw = DWP_FETCH(t), tn_raw = DWP_FETCH(t + nblocks), tp_raw = tc_raw, tnn_raw;
    DwpDesc tc = dwp_decode(tc_raw), tn = dwp_decode(tn_raw), tp = tc;
    tp.packed = 0;
    tp.szW = 0;

#define DWP_COLS(T) ((int)(((T).packed >> 8) & 0xFFu))
#define DWP_NBIAS(T) ((int)(((T).packed >> 16) & 0xFFu))
#define DWP_SZAB(T) ((((T).packed >> 24) & 1u) ? 0x7FFFFFFFu : 0u) /* operand reads never leave the allocation */
#define DWP_DIVN(x) (POW2 ? (x) * inv_nf : (x) / nf)
#define DWP_DIVN2(x) (POW2 ? (x) * inv2 : (x) / nf2)
    f32x2 mom2 = {mom, mom}, lr2 = {lr, lr}, wc2 = {wc, wc}, inv2 = {inv_nf, inv_nf}, nf2 = {nf, nf}, one2 = {1.0f, 1.0f};
    // Form of the update: the packed source (DWP_EPI_UPDATE) as the compiler lowers it by itself -- a mixture: it
    // scalarises the multiplies by the SGPR-held constants.  A scalar source and packed pairs with the constants
    // pinned in VGPR pairs evaluate the same IEEE operations per element (-ffp-contract=off: same bits) and measured
    // no faster (profiles/prologue_diet_update_forms.txt), so the form the kernel always had is the one that stays.
    // voffset of this lane's float4 number 0 of the wave tile of T, formed once per tile; OOB for the columns that do
    // not exist (a property of the lane).  Rows that do not exist need no test: the record's szW ends with the tile's
    // last real row (engine.hip dwp_table), so the hardware range check drops their stores and zeroes their loads.
    // float4 number IT is 8 rows further down: one add, kept in the VECTOR offset, which the range check always sees.
    // OOB + 24 rows stays beyond every descriptor (szW <= 256 Np) and below 2^31: Np < 2^17.
#define DWP_OFF0(T) ((32 * wn + 4 * ec) < DWP_COLS(T) ? (unsigned)(((32 * wm + er) * T.Np + 32 * wn + 4 * ec) * 4) : OOB)
#define DWP_OFF(BASE, T, IT) ((int)((BASE) + (unsigned)((IT) * 32 * T.Np)))
#define DWP_WRITE_UNIT(BUF)                                                                     \
    {                                                                                           \
        float *as = lds + (BUF)*8192, *bs = as + 4096;                                          \
        _Pragma("unroll") for (int q = 0; q < 4; q++) {                                         \
            *reinterpret_cast<float4 *>(as + (srow + 16 * q) * 64 + 4 * scol) = ra[q];          \
            *reinterpret_cast<float4 *>(bs + (srow + 16 * q) * 64 + 4 * scol) = rb[q];          \
        }                                                                                       \
    }
    // bias gradient of the tile's columns: frames summed sequentially in fp32 (kernAccSumrow order,
    // DevFunc.cu:267-285 <- BP_GPU.cu:434); the dEdX unit is in LDS anyway
#define DWP_BIAS(BUF, HH)                                                                       \
    {                                                                                           \
        if (tid < DWP_NBIAS(tc)) {                                                              \
            const float *col = lds + (BUF)*8192 + 4096 + tid;                                   \
            int bend = B - 64 * (HH);                                                           \
            bend = bend < 64 ? bend : 64;                                                       \
            /* opaque to the optimiser: hoisted out of the tile loop, the (uniform, loop-invariant) loop-entry test \
               below lives as a 64-bit lane mask in a scalar file that has no room for it -- a spill into VGPR     \
               lanes, read back inside the tile loop */                                         \
            asm volatile("" : "+s"(bend));                                                      \
            int b = 0;                                                                          \
            if ((HH) == 0) { /* B >= 1 (mlggd_create): frame 0 exists; no hoisted lane mask to keep live */ \
                bsum = col[0];                                                                  \
                b = 1;                                                                          \
            }                                                                                   \
            _Pragma("clang loop unroll(disable)") for (; b + 16 <= bend; b += 16) {             \
                float v[16];                                                                    \
                _Pragma("unroll") for (int u = 0; u < 16; u++) v[u] = col[(b + u) * 64];        \
                _Pragma("unroll") for (int u = 0; u < 16; u++) bsum += v[u];                    \
            }                                                                                   \
            _Pragma("clang loop unroll(disable)") for (; b < bend; b++) bsum += col[b * 64];    \
        }                                                                                       \
    }
    // bias update of the PREVIOUS tile (kernUpdatedelta with weightcost 0 + kernAccSum, BP_GPU.cu:435,437)
    // (buffer accesses, not pointer dereferences: a generic pointer out of the record compiles to FLAT loads /
    // stores, which return out of order and may alias LDS -- every later s_waitcnt in the tile then degrades to
    // vmcnt(0) / lgkmcnt(0) and the pipeline of the unit blocks is gone)
#define DWP_BIAS_UPDATE()                                                                       \
    {                                                                                           \
        if (tid < DWP_NBIAS(tp)) {                                                              \
            const DwpDesc tb_ = dwp_decode(tp_raw);                                             \
            const rsrc_t rb_ = make_rsrc(tb_.bias, 256), rdb_ = make_rsrc(tb_.dbias, FUSED ? 256 : 0); \
            if (FUSED) {                                                                        \
                const float bv = bload(rb_, tid * 4, 0);                                        \
                const float d = mom * bload(rdb_, tid * 4, 0) - lr * (DWP_DIVN(bsum_p) + 0.0f * bv); \
                bstore1(d, rdb_, tid * 4);                                                      \
                bstore1(d + 1.0f * bv, rb_, tid * 4);                                           \
            } else {                                                                            \
                bstore1(bsum_p, rb_, tid * 4);                                                  \
            }                                                                                   \
        }                                                                                       \
    }
    // epilogue of the previous tile, piece by piece.  Scratch word s of wave w -> row 4w + (s>>6&3) + 16*(s>>8),
    // column s&63 of the A half of buffer SB (the rows only wave w refills).
#define DWP_EPI_SCRATCH_WRITE(SB, R0, R1)                                                       \
    {                                                                                           \
        float *Tw = lds + (SB)*8192 + wave * 256;                                               \
        _Pragma("unroll") for (int r = (R0); r < (R1); r++) {                                   \
            const int kl = acc_row(r, lane);                                                    \
            Tw[(kl >> 3) * 1024 + ((kl >> 1) & 3) * 64 + (kl & 1) * 32 + i] = accp[r];          \
        }                                                                                       \
    }
    // (the empty asm with a "memory" clobber is a compiler-level fence that pins the read to the group it is written
    // in: left alone, the compiler sinks the LDS load down to its first use two groups later and then waits for it
    // with lgkmcnt(0) in front of an MFMA; the fence does not USE the value, so nothing waits for it here either)
#define DWP_EPI_SCRATCH_READ(SB, IT)                                                            \
    {                                                                                           \
        gq[IT] = *reinterpret_cast<const float4 *>(lds + (SB)*8192 + wave * 256 + (IT)*1024 + (er >> 1) * 64 + (er & 1) * 32 + 4 * ec); \
        asm volatile("" ::: "memory");                                                          \
    }
    // two weights per instruction (v_pk_mul_f32 / v_pk_add_f32: IEEE multiply / add per element, no contraction, so
    // the bits are those of the scalar expression): the fp32 MFMA occupies the SIMD's fp32 lanes, VALU work does
    // not hide behind it, and this halves the update's instruction count
#define DWP_EPI_UPDATE(PW, PD, IT)                                                              \
    {                                                                                           \
        const float4 gv_ = gq[IT];                                                              \
        const int off = DWP_OFF(offp_, tp, IT);                                                 \
        if (FUSED) { /* kernUpdatedelta (DevFunc.cu:502) then kernAccSum (DevFunc.cu:440) */ \
            const f32x2 w0 = {PW[IT].x, PW[IT].y}, w1 = {PW[IT].z, PW[IT].w};                   \
            f32x2 d0 = {PD[IT].x, PD[IT].y}, d1 = {PD[IT].z, PD[IT].w};                         \
            const f32x2 g0 = {gv_.x, gv_.y}, g1 = {gv_.z, gv_.w};                               \
            d0 = mom2 * d0 - lr2 * (DWP_DIVN2(g0) + wc2 * w0);                                  \
            d1 = mom2 * d1 - lr2 * (DWP_DIVN2(g1) + wc2 * w1);                                  \
            const f32x2 n0 = d0 + one2 * w0, n1 = d1 + one2 * w1;                               \
            bstore4(make_float4(d0.x, d0.y, d1.x, d1.y), rDp, off);                             \
            bstore4(make_float4(n0.x, n0.y, n1.x, n1.y), rWp, off);                             \
        } else {                                                                                \
            bstore4(gv_, rWp, off);                                                             \
        }                                                                                       \
    }
    long long ph_sum[5] = {0, 0, 0, 0, 0}, ph_last = 0;
#define DWP_PHASE(K)                                                                            \
    {                                                                                           \
        if (PHASES) {                                                                           \
            __builtin_amdgcn_sched_barrier(0);                                                  \
            const long long now_ = (long long)__builtin_amdgcn_s_memtime();                     \
            ph_sum[K] += now_ - ph_last;                                                        \
            ph_last = now_;                                                                     \
            __builtin_amdgcn_sched_barrier(0);                                                  \
        }                                                                                       \
    }
    // One 64-frame unit HH of the current tile, whose operands sit in LDS buffer BUF; the next unit's operands
    // (unit HH+1 of this tile, or unit 0 of the next) go to the other buffer.  PW / PD: the register set the pending
    // epilogue consumes (first unit) and the NEXT tile's W / delta are then loaded into (last unit).
#define DWP_UNIT(HH, BUF, PW, PD)                                                               \
    {                                                                                           \
        const bool FIRSTU = (HH) == 0, LASTU = (HH) == H - 1; /* constants once the unit loop is unrolled */ \
        DWP_BIAS(BUF, HH)                                                                       \
        if (FIRSTU) DWP_BIAS_UPDATE()                                                           \
        /* ---- one basic block from here to the barrier ---- */                                \
        const rsrc_t rA_ = LASTU ? make_rsrc(tn.A, DWP_SZAB(tn)) : make_rsrc(tc.A, DWP_SZAB(tc)); \
        const rsrc_t rB_ = LASTU ? make_rsrc(tn.Bm, DWP_SZAB(tn)) : make_rsrc(tc.Bm, DWP_SZAB(tc)); \
        const int ldA_ = LASTU ? tn.ldA : tc.ldA, ldB_ = LASTU ? tn.Np : tc.Np;                 \
        const int row0_ = LASTU ? 0 : 64 * ((HH) + 1);                                          \
        /* LDS-DMA offsets: the lane's part once per unit, the wave-uniform row part in soffset (these loads rely   \
           only on the all-or-nothing DWP_SZAB descriptor, which no offset can leave) */        \
        const int voA_ = (srow * ldA_ + 4 * scol) * 4, voB_ = (srow * ldB_ + 4 * scol) * 4;     \
        const rsrc_t rWn = make_rsrc(tn.W, tn.szW), rDn = make_rsrc(tn.D, FUSED ? tn.szW : 0);  \
        const rsrc_t rWp = make_rsrc(tp.W, tp.szW), rDp = make_rsrc(tp.D, FUSED ? tp.szW : 0);  \
        const unsigned offp_ = FIRSTU ? DWP_OFF0(tp) : 0u, offn_ = (FUSED && LASTU) ? DWP_OFF0(tn) : 0u; \
        const float *ap = lds + (BUF)*8192 + h5 * 64 + 32 * wm + i;                             \
        const float *bp = lds + (BUF)*8192 + 4096 + h5 * 64 + 32 * wn + i;                      \
        float fa[32], fb[32]; /* static indices only: registers */                              \
        float4 gq[4];                                                                           \
        /* (BIAS_ONLY: constants nobody reads; leaving fa / fb unset instead reorders k_dwp_bias's instructions) */ \
        _Pragma("unroll") for (int p = 0; p < 4; p++) {                                         \
            fa[p] = BIAS_ONLY ? 1.0f : ap[p * 128];                                             \
            fb[p] = BIAS_ONLY ? 1.0f : bp[p * 128];                                             \
        }                                                                                       \
        if (FIRSTU) tnn_raw = DWP_FETCH(t + 2 * nblocks);                                       \
        __builtin_amdgcn_sched_barrier(0);                                                      \
        _Pragma("unroll") for (int g = 0; g < 16; g++) {                                        \
            if (!BIAS_ONLY) {                                                                   \
                acc = mfma32(fa[2 * g], fb[2 * g], acc);                                        \
                acc = mfma32(fa[2 * g + 1], fb[2 * g + 1], acc);                                \
            }                                                                                   \
            if (g < 14 && !BIAS_ONLY) {                                                         \
                _Pragma("unroll") for (int p = 2 * g + 4; p < 2 * g + 6; p++) {                 \
                    fa[p] = ap[p * 128];                                                        \
                    fb[p] = bp[p * 128];                                                        \
                }                                                                               \
            }                                                                                   \
            /* operands of the next unit straight into LDS by LDS-DMA (buffer_load ... lds), one 16-byte load per  \
               lane and instruction: no staging registers (-28 VGPRs) and no ds_write_b128, -2.4 % launch time      \
               against loading into registers and writing LDS in groups 12..15.  All of them are OLDER than the     \
               pending epilogue's last stores (group 10): s_waitcnt vmcnt counts in issue order, and the hand-off   \
               below must not have to wait for a store to be acknowledged.                      \
               Wave w's 64 lanes fill rows 4w..4w+3 (+16q) of the A / B halves, 1 KB contiguous per instruction,   \
               which is exactly the row-major layout the fragment reads expect.  In the unit that carries a         \
               pending epilogue the A rows are its scratch, so they are filled only after the scratch has been      \
               read back (groups 6..9); the B rows go first (groups 0..3). */                    \
            {                                                                                   \
                const int qa = FIRSTU ? g - 6 : g, qb = FIRSTU ? g : g - 4;                     \
                if (qa >= 0 && qa < 4) {                                                        \
                    float *dst = lds + ((BUF) ^ 1) * 8192 + (4 * wave + 16 * qa) * 64;          \
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rA_, (__attribute__((address_space(3))) void *)dst, 16, \
                                                             voA_, (row0_ + 16 * qa) * ldA_ * 4, 0, 0);  \
                }                                                                               \
                if (qb >= 0 && qb < 4) {                                                        \
                    float *dst = lds + ((BUF) ^ 1) * 8192 + 4096 + (4 * wave + 16 * qb) * 64;   \
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rB_, (__attribute__((address_space(3))) void *)dst, 16, \
                                                             voB_, (row0_ + 16 * qb) * ldB_ * 4, 0, 0);  \
                }                                                                               \
            }                                                                                   \
            /* epilogue of the previous tile: accumulators -> scratch (groups 0, 1), read back (float4 IT in group    \
               2 + IT), update + stores (group 4 + 2 IT: every read is at least two groups old when it is used) */ \
            if (FIRSTU) {                                                                       \
                if (g == 0) DWP_EPI_SCRATCH_WRITE((BUF) ^ 1, 0, 8)                              \
                if (g == 1) {                                                                   \
                    DWP_EPI_SCRATCH_WRITE((BUF) ^ 1, 8, 16)                                     \
                    __builtin_amdgcn_wave_barrier();                                            \
                }                                                                               \
                if (g >= 2 && g <= 5) DWP_EPI_SCRATCH_READ((BUF) ^ 1, g - 2)                    \
                if (g >= 4 && g <= 10 && (g & 1) == 0 && !BIAS_ONLY) DWP_EPI_UPDATE(PW, PD, (g - 4) >> 1) \
            }                                                                                   \
            /* W / delta of the NEXT tile, consumed by its epilogue a whole tile later: into the set the pending       \
               epilogue has just used (groups 12..15 when this unit is both first and last, else one load per group    \
               8..15) */                                                                        \
            if (FUSED && LASTU && !BIAS_ONLY) {                                                 \
                if (FIRSTU) {                                                                   \
                    if (g >= 12) {                                                              \
                        PW[g - 12] = bload4(rWn, DWP_OFF(offn_, tn, g - 12), 0);                \
                        PD[g - 12] = bload4(rDn, DWP_OFF(offn_, tn, g - 12), 0);                \
                    }                                                                           \
                } else if (g >= 8) {                                                            \
                    if (g < 12) PW[g - 8] = bload4(rWn, DWP_OFF(offn_, tn, g - 8), 0);          \
                    else PD[g - 12] = bload4(rDn, DWP_OFF(offn_, tn, g - 12), 0);               \
                }                                                                               \
            }                                                                                   \
            __builtin_amdgcn_sched_barrier(0);                                                  \
        }                                                                                       \
        DWP_PHASE(LASTU ? 2 : 0)                                                                \
        {                                                                                       \
            /* every wave's own DMA has to have landed before the barrier lets the others read its rows: wait for   \
               all vector-memory operations but the ones issued after the last DMA of this unit (vmcnt counts in     \
               issue order): first unit: the stores of group 10 (2 FUSED, else 1; + 8 W / delta loads of groups     \
               12..15 when it is also the last); other last units: 8 W / delta loads; otherwise none */ \
            const int younger = FIRSTU ? ((FUSED ? 2 : 1) + ((LASTU && FUSED) ? 8 : 0)) : ((LASTU && FUSED) ? 8 : 0); \
            if (younger == 0) __builtin_amdgcn_s_waitcnt(0x0F70);                               \
            else if (younger == 1) __builtin_amdgcn_s_waitcnt(0x0F71);                          \
            else if (younger == 2) __builtin_amdgcn_s_waitcnt(0x0F72);                          \
            else if (younger == 8) __builtin_amdgcn_s_waitcnt(0x0F78);                          \
            else __builtin_amdgcn_s_waitcnt(0x0F7A);                                            \
        }                                                                                       \
        __syncthreads();                                                                        \
        DWP_PHASE(LASTU ? 4 : 1)                                                                \
    }
    // one tile whose first unit sits in LDS buffer BASE
#define DWP_TILE(BASE, PW, PD)                                                                  \
    {                                                                                           \
        _Pragma("unroll") for (int hh = 0; hh < H; hh++) DWP_UNIT(hh, ((BASE) + hh) & 1, PW, PD) \
        /* the tile's accumulators, bias sum and record become "previous": their epilogue rides in the next tile */ \
        accp = acc;                                                                             \
        _Pragma("unroll") for (int r = 0; r < 16; r++) acc[r] = 0.0f;                           \
        bsum_p = bsum;                                                                          \
        tp = tc;                                                                                \
        tp_raw = tc_raw;                                                                        \
        t += nblocks;                                                                           \
        if (t >= total) break;                                                                  \
        tc = tn;                                                                                \
        tc_raw = tn_raw;                                                                        \
        tn = dwp_decode(tnn_raw);                                                               \
        tn_raw = tnn_raw;                                                                       \
    }

    // prologue: first unit into buffer 0, the first tile's W / delta into set 0
    {
        const rsrc_t rA_ = make_rsrc(tc.A, DWP_SZAB(tc)), rB_ = make_rsrc(tc.Bm, DWP_SZAB(tc));
        const rsrc_t rWc = make_rsrc(tc.W, tc.szW), rDc = make_rsrc(tc.D, FUSED ? tc.szW : 0);
        const unsigned offc_ = DWP_OFF0(tc);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = srow + 16 * q;
            ra[q] = bload4(rA_, (row * tc.ldA + 4 * scol) * 4, 0);
            rb[q] = bload4(rB_, (row * tc.Np + 4 * scol) * 4, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            pw0[q] = FUSED ? bload4(rWc, DWP_OFF(offc_, tc, q), 0) : make_float4(0.f, 0.f, 0.f, 0.f);
            pd0[q] = FUSED ? bload4(rDc, DWP_OFF(offc_, tc, q), 0) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    DWP_WRITE_UNIT(0)
    __syncthreads();
    if (PHASES) ph_last = (long long)__builtin_amdgcn_s_memtime();
    // a tile of H units leaves its successor's first unit in buffer (BASE + H) & 1
    // tile k of this workgroup: its pending epilogue (tile k-1) consumes set (k-1) & 1, which its last unit refills
    // with tile k+1's W / delta; set k & 1 (loaded during tile k-1, or in the prologue) waits for tile k+1
    bool last_set1 = true;
    for (;;) {
        last_set1 = false;  // the tile that ends the walk here leaves ITS W / delta in set 0
        DWP_TILE(0, pw1, pd1)
        last_set1 = true;
        DWP_TILE(H & 1, pw0, pd0)
    }
    // epilogue of the last tile (tp): nothing left to hide it behind.  Both operand buffers are dead (every wave has
    // passed the last unit's barrier) and the scratch rows are wave-private.
    {
        DWP_BIAS_UPDATE()
        const rsrc_t rWp = make_rsrc(tp.W, tp.szW), rDp = make_rsrc(tp.D, FUSED ? tp.szW : 0);
        const unsigned offp_ = DWP_OFF0(tp);
        float4 gq[4];
        DWP_EPI_SCRATCH_WRITE(0, 0, 16)
        __builtin_amdgcn_wave_barrier();
        _Pragma("unroll") for (int it = 0; it < 4; it++) DWP_EPI_SCRATCH_READ(0, it)
        if (last_set1) {
            _Pragma("unroll") for (int it = 0; it < 4; it++) DWP_EPI_UPDATE(pw1, pd1, it)
        } else {
            _Pragma("unroll") for (int it = 0; it < 4; it++) DWP_EPI_UPDATE(pw0, pd0, it)
        }
    }
    stamp_clk(stamps, 2, bid);
    if (stamps != nullptr && threadIdx.x == 0) stamps[(size_t)bid * 8 + 4] = (t - bid) / nblocks;  // tiles walked
    if (PHASES && stamps != nullptr && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 5; k++) stamps[(size_t)(nblocks + bid) * 8 + k] = ph_sum[k];
    }
#undef DWP_PHASE
#undef DWP_FETCH
#undef DWP_WRITE_UNIT
#undef DWP_OFF
#undef DWP_OFF0
#undef DWP_BIAS
#undef DWP_BIAS_UPDATE
#undef DWP_EPI_SCRATCH_WRITE
#undef DWP_EPI_SCRATCH_READ
#undef DWP_EPI_UPDATE
#undef DWP_UNIT
#undef DWP_TILE
#undef DWP_COLS
#undef DWP_NBIAS
#undef DWP_SZAB
#undef DWP_DIVN
#undef DWP_DIVN2
}

// ---------------------------------------------------------------------------------------
// Launch wrappers.  The bodies above are __device__ functions taking an explicit block id
// and LDS base so that several of them can share one launch.  That was tried -- dX(l) together
// with dW(l+1), and forward_1 of the next minibatch with dW(2), as two roles of one grid so an
// MFMA-bound and an HBM-bound body share every CU -- and measured at exactly the sum of the
// separate launches (they contend in the CU's memory pipeline instead of complementing each
// other), so only the stand-alone kernels remain.
// ---------------------------------------------------------------------------------------
extern __shared__ __attribute__((aligned(16))) float g_dyn_lds[];

// STAMPED: the diagnostic form, launched only for the one launch mlggd_debug_stamp_select() picked.  The normal
// form ignores `stamps` altogether: a null test at the top of a kernel splits its argument loads into two dependent
// groups (test the pointer, branch, only then fetch the rest), a second memory round trip in front of the first
// operand load of every launch.
template <int MODE, int NW, int PIPE = 1, bool STAMPED = false>
__global__ __launch_bounds__(64 * NW) void k_fwd(FwdArgs A, long long *stamps) {
    fwd_body<MODE, NW, PIPE>(A, (int)blockIdx.x, g_dyn_lds, STAMPED ? stamps : nullptr);
}
template <int NW, int PIPE = 1, int ACT = ACT_SIGMOID, bool STAMPED = false>
__global__ __launch_bounds__(64 * NW) void k_dx(DxArgs A, long long *stamps) {
    dx_body<NW, PIPE, ACT>(A, (int)blockIdx.x, g_dyn_lds, STAMPED ? stamps : nullptr);
}
#include "kernels64.hip.h"  // k_fwd64 / k_dx64: the 64 x 64-tile forms for large minibatches
template <int H, bool FUSED, bool POW2, bool STAMPED = false>
__global__ __launch_bounds__(256) void k_dwp(const DwpDesc *__restrict__ table, int total, DwpConst C, long long *stamps) {
    dwp_body<H, FUSED, POW2>(table, total, C, (int)blockIdx.x, (int)gridDim.x, g_dyn_lds, STAMPED ? stamps : nullptr);
}
// Bias-only tiles (sharded data parallel: the tiles of weight-row block 0 on the ranks that do not own it, so that
// every rank applies the identical bias update without another collective): the same walk with everything but the
// operand staging and the bias gradient / update compiled out -- no W / delta access, no fragment reads, no MFMAs.
// They get a launch of their own: inside the main launch the skip would be a branch around the MFMAs, which splits
// the unit blocks and undoes the interleave for every tile (what slowed the round-1 kernel down).
template <int H, bool POW2>
__global__ __launch_bounds__(256) void k_dwp_bias(const DwpDesc *__restrict__ table, int total, DwpConst C, long long *stamps) {
    dwp_body<H, true, POW2, false, true>(table, total, C, (int)blockIdx.x, (int)gridDim.x, g_dyn_lds, nullptr);
}
// diagnostic twin of k_dwp<H, true, true> with the per-phase cycle sums (never launched unless asked for)
template <int H>
__global__ __launch_bounds__(256) void k_dwp_phases(const DwpDesc *__restrict__ table, int total, DwpConst C, long long *stamps) {
    dwp_body<H, true, true, true>(table, total, C, (int)blockIdx.x, (int)gridDim.x, g_dyn_lds, stamps);
}
// Elementwise update from an (all-reduced) gradient, data-parallel path.  Pad entries have
// G = delta = W = 0 and stay 0.  kernUpdatedelta + kernAccSum, DevFunc.cu:490-507,427-443.
__global__ __launch_bounds__(256) void k_apply_update(float *__restrict__ Wt, float *__restrict__ delta,
                                                      const float *__restrict__ G, size_t n4, float nf, float mom,
                                                      float lr, float wc) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n4; idx += stride) {
        const float4 g = reinterpret_cast<const float4 *>(G)[idx];
        float4 w = reinterpret_cast<float4 *>(Wt)[idx];
        float4 d = reinterpret_cast<float4 *>(delta)[idx];
        d.x = mom * d.x - lr * (g.x / nf + wc * w.x);
        d.y = mom * d.y - lr * (g.y / nf + wc * w.y);
        d.z = mom * d.z - lr * (g.z / nf + wc * w.z);
        d.w = mom * d.w - lr * (g.w / nf + wc * w.w);
        w.x = d.x + 1.0f * w.x;
        w.y = d.y + 1.0f * w.y;
        w.z = d.z + 1.0f * w.z;
        w.w = d.w + 1.0f * w.w;
        reinterpret_cast<float4 *>(delta)[idx] = d;
        reinterpret_cast<float4 *>(Wt)[idx] = w;
    }
}

// Diagnostic (mlggd_debug_math): the device's own libm calls of the loss / activation epilogues applied to an
// array, so a test can measure in ulps how far ocml's powf / expf sit from the correctly rounded result and from
// the oracle's glibc -- the only arithmetic of the loss chain that is not IEEE-exact on both sides.
//   fn 0: powf(x, y)   1: expf(x) (ocml; no kernel uses it any more)   2: sigmoid_det(x), the forward epilogues' sigmoid
//   3: x / y   4: exp_det(x)   5: pow_det(x, y), the loss chain's power   6: the packed form of the sigmoid (sigmoid_det4)
//   7: relu4(x), the rectifier of the FWD_RELU epilogues
__global__ __launch_bounds__(256) void k_debug_math(int fn, const float *__restrict__ x, float y, float *__restrict__ out,
                                                    size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    out[i] = fn == 0 ? powf(v, y) : fn == 1 ? expf(v) : fn == 2 ? sigmoid_det(v) : fn == 6 ? sigmoid_det4(make_float4(v, v, v, v), 0.0f, true).z : fn == 7 ? relu4(make_float4(v, v, v, v), 0.0f, true).z : fn == 4 ? exp_det(v) : fn == 5 ? pow_det(v, y) : v / y;
}

// keeps one wave busy for `ticks` of the 100 MHz wall clock (bounded: at most `ticks` iterations of a loop whose
// body takes longer than a tick): engine.hip create_concurrent_stream probes with it whether a new stream runs beside
// the main stream or behind it
__global__ __launch_bounds__(64) void k_spin(long long ticks) {
    const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
    for (long long i = 0; i < ticks; i++) {
        if ((long long)__builtin_amdgcn_s_memrealtime() - t0 >= ticks) break;
        __builtin_amdgcn_s_sleep(8);
    }
}

// does nothing: the kernel mlggd_profile_overhead brackets to calibrate what a HIP-event bracket costs by itself
__global__ __launch_bounds__(256) void k_nop() {}

// dst = a + b elementwise (a == nullptr: dst = b).  Only the one-GPU emulation of the data-parallel
// exchange uses it (mlggd_debug_fake_world: the sum over emulated ranks that a collective would form).
__global__ __launch_bounds__(256) void k_accum(float *__restrict__ dst, const float *a, const float *b, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride)
        dst[idx] = a ? a[idx] + b[idx] : b[idx];
}

// ---------------------------------------------------------------------------------------
// Bias update from the all-reduced bias gradients of every layer in one launch
// (data-parallel path only; on one GPU the bias gradient and update live in k_dw):
// kernUpdatedelta with weightcost 0 and kernAccSum (BP_GPU.cu:435,437).
// ---------------------------------------------------------------------------------------
struct BiasJob {
    const float *dEdX;  // [Bp][Np]
    float *bias, *dbias, *gb;
    int N, Np, first;   // first = prefix offset of this layer in the flattened unit index
};
struct BiasJobs {
    BiasJob job[10];
    int njobs, total;
};

__global__ __launch_bounds__(256) void k_bias_apply(BiasJobs jobs, float nf, float mom, float lr) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= jobs.total) return;
    int j = 0;
#pragma unroll
    for (int q = 1; q < 10; q++)
        if (q < jobs.njobs && g >= jobs.job[q].first) j = q;
    const BiasJob jb = jobs.job[j];
    const int n = g - jb.first;
    if (n >= jb.N) return;
    const float bv = jb.bias[n];
    const float d = mom * jb.dbias[n] - lr * (jb.gb[n] / nf + 0.0f * bv);
    jb.dbias[n] = d;
    jb.bias[n] = d + 1.0f * bv;
}

// ---------------------------------------------------------------------------------------
// The Adam rule (adam_rule.h, mlggd_set_optimizer) on every layer's padded weight matrix and every bias vector in one
// launch, from the gradients the unfused dW launches wrote: reads G, W, m, v, writes W, m, v, 16 bytes per lane and
// array.  A job is one array of n4 float4 (a whole padded [Kp][Np] matrix, or the Np entries of a bias: pads hold
// G = w = m = v = 0 and stay 0); the jobs' chunks of 256 float4 are numbered through, `first` being a job's first chunk,
// so a workgroup's chunk belongs to one job and the look-up is scalar.  Grid-stride over the chunks under a capped grid.
// ---------------------------------------------------------------------------------------
#define ADAM_MAXJOBS 18  // 2 (MLGGD_MAXLAYER - 1): weights and bias of every layer
struct AdamJob {
    float *w, *m, *v;
    const float *G;
    unsigned n4;     // float4 of the array
    unsigned first;  // chunks of 256 float4 in front of this job
    float wc;        // weightcost; 0 for a bias
    int pad_;
};
struct AdamJobs {
    AdamJob job[ADAM_MAXJOBS];
    int njobs;
    unsigned chunks;  // of all jobs
};

__global__ __launch_bounds__(256) void k_adam_apply(AdamJobs jobs, adam_rule::Consts c) {
    for (unsigned ch = blockIdx.x; ch < jobs.chunks; ch += gridDim.x) {
        int j = 0;
        for (int q = 1; q < jobs.njobs; q++)
            if (ch >= jobs.job[q].first) j = q;
        const AdamJob jb = jobs.job[j];
        const unsigned idx = (ch - jb.first) * 256u + threadIdx.x;
        if (idx >= jb.n4) continue;
        const float4 g = reinterpret_cast<const float4 *>(jb.G)[idx];
        float4 w = reinterpret_cast<float4 *>(jb.w)[idx];
        float4 m = reinterpret_cast<float4 *>(jb.m)[idx];
        float4 v = reinterpret_cast<float4 *>(jb.v)[idx];
        const adam_rule::Moments x = adam_rule::step(w.x, m.x, v.x, g.x, jb.wc, c);
        const adam_rule::Moments y = adam_rule::step(w.y, m.y, v.y, g.y, jb.wc, c);
        const adam_rule::Moments z = adam_rule::step(w.z, m.z, v.z, g.z, jb.wc, c);
        const adam_rule::Moments u = adam_rule::step(w.w, m.w, v.w, g.w, jb.wc, c);
        reinterpret_cast<float4 *>(jb.w)[idx] = make_float4(x.w, y.w, z.w, u.w);
        reinterpret_cast<float4 *>(jb.m)[idx] = make_float4(x.m, y.m, z.m, u.m);
        reinterpret_cast<float4 *>(jb.v)[idx] = make_float4(x.v, y.v, z.v, u.v);
    }
}

// ---------------------------------------------------------------------------------------
// Input staging: row b of the minibatch -> inT[k][b], padded with zeros (k >= K or b >= B).
// 32x32 tiles through LDS; both sides coalesced.  Two sources (Interface::Readchunk,
// Interface.cc:778-785, builds row b as the fea_context consecutive frames of one window):
//   first == nullptr : the caller's expanded chunk, row b at in + b*ld           (BP_GPU::train)
//   first != nullptr : the raw frame stream; row b is the contiguous slice that starts at frame
//                      first[b], i.e. in + first[b]*fdim  (the window IS consecutive frames, so
//                      nothing has to be expanded on the host).
// Either way the rows are also written row-major to rows_out[b][Kp] (row stride Kp = ceil32(K), zeros in
// the pad columns and pad rows): the layer-1 operand of the dW kernel.  The caller's rows have a stride of K
// floats -- 2827 is odd, so three rows out of four start off a 16-byte boundary and every 16-byte load of
// the dW kernel from them splits -- the copy costs 1.4 MB of writes in a kernel that touches every element anyway.
// ---------------------------------------------------------------------------------------
struct StageArgs {
    const float *in;
    int ld, B, K, Kp;
    float *inT;
    int Bp, b_tiles;
    const int *first;
    int fdim;
    float *rows_out;
    int yblk;  // 0: rows_out is row-major [Bp][Kp]; > 0: blocked by owner, [Kp / yblk blocks][Bp][yblk] (y_blocked_base)
};
// SUB: 256-thread staging tiles per workgroup (1: the workgroup is one tile; 4: a 1024-thread workgroup stages tiles
// 4*bid .. 4*bid+3, of which the ones past n_tiles do nothing but keep the barrier company)
template <int SUB = 1>
__device__ __forceinline__ void transpose_in_body(const StageArgs &A, const int bid, const int n_tiles = 0x7FFFFFFF) {
    const float *__restrict__ in = A.in;
    float *__restrict__ inT = A.inT, *__restrict__ rows_out = A.rows_out;
    const int *__restrict__ first = A.first;
    const int ld = A.ld, B = A.B, K = A.K, Bp = A.Bp, b_tiles = A.b_tiles, fdim = A.fdim;
    __shared__ float ts[SUB][32][33];
    const int sub = SUB == 1 ? 0 : (int)(threadIdx.x >> 8), tile = SUB * bid + sub;
    float(*t)[33] = ts[sub];
    const bool live = tile < n_tiles;
    const int kt = tile / b_tiles, bt = tile % b_tiles;
    const int k0 = kt * 32, b0 = bt * 32;
    const int tx = threadIdx.x & 31, ty = (threadIdx.x >> 5) & 7;
    if (live) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int b = b0 + ty + 8 * q, k = k0 + tx;
            float v = 0.0f;
            if (b < B && k < K) {
                const size_t base = first ? (size_t)first[b] * fdim : (size_t)b * ld;
                v = in[base + k];
            }
            if (rows_out) {  // b < Bp, k < Kp: the grid's tiles cover exactly that
                if (A.yblk) rows_out[y_blocked_base(k0, A.yblk, Bp) + (size_t)b * A.yblk + tx] = v;
                else rows_out[(size_t)b * A.Kp + k] = v;
            }
            t[ty + 8 * q][tx] = v;
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = k0 + ty + 8 * q;
            inT[(size_t)k * Bp + b0 + tx] = t[tx][ty + 8 * q];
        }
    }
}
__global__ __launch_bounds__(256) void k_transpose_in(StageArgs A) { transpose_in_body(A, (int)blockIdx.x); }

// Input staging of a noise-aware (NAT) engine, nat_rule.h: row b is its window of the frame stream, K - fdim columns
// from in + first[b] * fdim as above, followed by the fdim values of its utterance's noise row, nat + nat_row[b] * fdim.
// The same 32 x 32 LDS tiles, grid and outputs as k_transpose_in (inT, rows_out in either form, zero pads); a launch of
// its own in front of the forward pass -- the loss kernels stage the plain form only.  A.first is never NULL here.
__global__ __launch_bounds__(256) void k_transpose_in_nat(StageArgs A, const float *__restrict__ nat,
                                                          const int *__restrict__ nat_row) {
    const float *__restrict__ in = A.in;
    float *__restrict__ inT = A.inT, *__restrict__ rows_out = A.rows_out;
    const int *__restrict__ first = A.first;
    const int B = A.B, K = A.K, Bp = A.Bp, b_tiles = A.b_tiles, fdim = A.fdim, Kwin = A.K - A.fdim;
    __shared__ float t[32][33];
    const int tile = (int)blockIdx.x;
    const int kt = tile / b_tiles, bt = tile % b_tiles;
    const int k0 = kt * 32, b0 = bt * 32;
    const int tx = threadIdx.x & 31, ty = (threadIdx.x >> 5) & 7;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int b = b0 + ty + 8 * q, k = k0 + tx;
        float v = 0.0f;
        if (b < B && k < K) {
            if (k < Kwin) v = in[(size_t)first[b] * fdim + k];
            else v = nat[(size_t)nat_row[b] * fdim + (k - Kwin)];
        }
        if (rows_out) {  // b < Bp, k < Kp: the grid's tiles cover exactly that
            if (A.yblk) rows_out[y_blocked_base(k0, A.yblk, Bp) + (size_t)b * A.yblk + tx] = v;
            else rows_out[(size_t)b * A.Kp + k] = v;
        }
        t[ty + 8 * q][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int k = k0 + ty + 8 * q;
        inT[(size_t)k * Bp + b0 + tx] = t[tx][ty + 8 * q];
    }
}

// The noise rows of a batch, nat_rule.h: one ordered chain per (utterance, bin).  rows [sum F][D] are the packed frames
// of n_utts utterances, utterance u's from frame_off[u]; mean == nullptr: the rows are already normalised, else they are
// LPS rows and every term is (lps - mean) * inv first.  out [n_utts][D]; an utterance without frames gets zeros.
__global__ __launch_bounds__(256) void k_nat_estimate(const float *__restrict__ rows, const int *__restrict__ frame_off,
                                                      int n_utts, int D, int T, const float *__restrict__ mean,
                                                      const float *__restrict__ inv, float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_utts * D) return;
    const int u = (int)(i / D), k = (int)(i % D);
    const int fo = frame_off[u], Tu = nat_rule::frames_used(T, frame_off[u + 1] - fo);
    const float *x = rows + (size_t)fo * D + k;
    out[i] = mean ? nat_rule::chain_lps(x, (size_t)D, Tu, mean[k], inv[k]) : nat_rule::chain(x, (size_t)D, Tu);
}

// nat_row of a decoding chunk: sample i is packed frame a + i, its noise row is its utterance's (frame_off strictly
// increasing over the n_utts utterances; utt_of, when given, is the per-frame table of the same answer)
__global__ __launch_bounds__(256) void k_nat_rows_seg(const int *__restrict__ frame_off, const int *__restrict__ utt_of,
                                                      int n_utts, int a, int n, int *__restrict__ nat_row) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    if (utt_of) {
        nat_row[i] = utt_of[a + i];
        return;
    }
    int lo = 0, hi = n_utts - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frame_off[mid] <= a + i) lo = mid;
        else hi = mid - 1;
    }
    nat_row[i] = lo;
}

// Sum of the S split-K slabs of one output element, slabs added in order s = 0..S-1.  All
// loads are issued before the first add (one memory round trip instead of S).
__device__ __forceinline__ float slab_sum(const float *__restrict__ slab, size_t o, size_t stride, int S) {
    float v[8];
#pragma unroll
    for (int s = 0; s < 8; s++) v[s] = slab[(size_t)(s < S ? s : 0) * stride + o];
    float x = v[0];
#pragma unroll
    for (int s = 1; s < 8; s++)
        if (s < S) x += v[s];
    for (int s = 8; s < S; s++) x += slab[(size_t)s * stride + o];
    return x;
}

// ---------------------------------------------------------------------------------------
// Output-layer loss kernels.  One workgroup = 8 output units (d) x 32 frames (b), ONE element per thread, lanes
// along the frames: the slab / outT / eT / pT / dEdXt rows are read and written in 128-byte segments; targ and
// the row-major dEdX are touched in 32-byte pieces (they are 0.13 MB per step).  Round 1 used 32 x 32 tiles with
// four elements per thread: 36 workgroups whose threads each ran four slab sums and four powf one after the other
// -- 8 us of pure latency for 33k elements; with 144 workgroups the chain is a quarter as long.
// pow(x, 1.0f) is x itself and pow(x, 0.0f) is 1 for every float (IEEE 754-2008 9.2.1 / C99 F.9.4.4): the correctly
// rounded results, which glibc's powf (the oracle) returns.  EVERY pow of the chain goes through pow_or_self, so at
// the reference's shipped objective (MLflag = 1, shapefactor = 1, TC/finetune.pl:25-26) the chain holds no libm call
// at all -- p = |e|, alpha = v2, alpha^beta = alpha, |e|^(beta-1) = 1 -- and is IEEE arithmetic in the reference's
// order; the same for the MMSE case (beta - 1 = 1).  What ocml's powf itself returns for y = 1 and y = 0 is measured
// in tests/test_gpu_loss_ulps.py.
// ---------------------------------------------------------------------------------------
constexpr int LOSS_DT = 8;  // output units per loss workgroup
// For every other exponent: pow_det (defined beside exp_det above).
__device__ __forceinline__ float pow_or_self(float x, float p) { return p == 1.0f ? x : p == 0.0f ? 1.0f : pow_det(x, p); }

// Phase A:   out = bias + sum_s slab;  e = out - targ;  p = |e|^beta
// kernerror, kernabsolutevalus, kernindex2 (DevFunc.cu:399-409,186-191,219-227 <- BP_GPU.cu:413-415).
// Writes outT, eT, pT, all [Dp][Bp] with zeros in the pads.
struct LossErrArgs {
    const float *slab;
    int S;
    const float *bias, *targ;
    int B, D, Dp, Bp;
    float beta;
    int want_pow;
    float *outT, *eT, *pT;
    int b_tiles;
    const int *first;
    int toff;
};
// The error model of the output-layer loss, a compile-time tag.  The families below (loss_err, loss_grad, loss_ml,
// cv_reduce) are ONE body each, instantiated per model, and the models substitute exactly three things:
//   EM_SHARED  the reference's scalar shape: beta is the argument struct's (A.beta), the magnitude of an error is
//              fabsf(e), the gradient takes its sign from the three-way if of kernfunc2;
//   EM_BINS    a shape per output unit (mlggd_set_shapefactors): beta_d from betas [Dp] (pads 1.0), the rest as EM_SHARED;
//   EM_ASYM    a shape and a skew per unit (mlggd_set_asymmetry, asym_rule.h): beta_d as EM_BINS (an engine without a
//              shape vector fills betas with cfg.shapefactor), kappa_d from kappas [Dp] (pads 1.0), the magnitude is
//              s(e) = kappa_d e (e > 0), (-e) / kappa_d (e < 0), and the gradient is the existing value at s(e) times
//              ds/de (asym_rule::grad).  s and the choice between the two gradient forms are selects on the lane's
//              own e; beta and kappa are uniform over a unit's lanes, so pow_or_self's branches stay uniform.  At
//              kappa = 1 every intermediate is EM_BINS' value.  ML only: there is no want_pow and no MLflag.
// A model's pointers are nullptr where it does not read them.  Every other statement -- slab sum, target gather,
// kernSumcol's order, alpha and alpha^beta, LDS layout, stores, reductions -- is the same text for all three.
enum ErrModel { EM_SHARED, EM_BINS, EM_ASYM };
// Phase A is the one family whose EM_ASYM instantiation of a shared body does not compile to the code its own kernel
// has (the target row's 64-bit index costs five more integer instructions, profiles/loss_family_isa.txt), so
// k_loss_err_asym below keeps its own text and this body serves EM_SHARED and EM_BINS.
template <int EM>
__device__ __forceinline__ void loss_err_body(const LossErrArgs &A, const float *__restrict__ betas, const int bid) {
    static_assert(EM != EM_ASYM, "k_loss_err_asym has its own text");
    const float *__restrict__ slab = A.slab, *__restrict__ bias = A.bias, *__restrict__ targ = A.targ;
    float *__restrict__ outT = A.outT, *__restrict__ eT = A.eT, *__restrict__ pT = A.pT;
    const int *__restrict__ first = A.first;
    // first != nullptr: targ is the raw target frame stream and sample b's target is frame
    // first[b] + toff of it (Interface.cc:822-825); otherwise row b of the caller's [B][D] matrix
    const int dt = bid / A.b_tiles, bt = bid % A.b_tiles;
    const int d = dt * LOSS_DT + (int)(threadIdx.x >> 5), b = bt * 32 + (int)(threadIdx.x & 31);
    const size_t o = (size_t)d * A.Bp + b;
    float x = slab_sum(slab, o, (size_t)A.Dp * A.Bp, A.S);
    x = x + bias[d];
    float e = 0.0f, p = 0.0f;
    if (b < A.B && d < A.D) {
        e = x - targ[(size_t)(first ? first[b] + A.toff : b) * A.D + d];  // kernerror
        if (A.want_pow) p = pow_or_self(fabsf(e), EM == EM_SHARED ? A.beta : betas[d]);  // kernabsolutevalus + kernindex2
    } else {
        x = 0.0f;
    }
    outT[o] = x;
    eT[o] = e;
    pT[o] = p;
}
// The blocks past n_loss stage the NEXT minibatch's input (it depends on nothing in this step and
// Yt[0] is free once forward_1 has run): the loss workgroups occupy a fraction of the CUs, so the staging
// blocks ride along on the idle ones instead of costing a launch of their own.
__global__ __launch_bounds__(256) void k_loss_err(LossErrArgs A, int n_loss, StageArgs G) {
    const int n_stage = (int)gridDim.x - n_loss;  // staging blocks first: they are the longer ones
    if ((int)blockIdx.x >= n_stage) loss_err_body<EM_SHARED>(A, nullptr, (int)blockIdx.x - n_stage);
    else transpose_in_body(G, (int)blockIdx.x);
}
__global__ __launch_bounds__(256) void k_loss_err_bins(LossErrArgs A, const float *__restrict__ betas, int n_loss,
                                                       StageArgs G) {
    const int n_stage = (int)gridDim.x - n_loss;
    if ((int)blockIdx.x >= n_stage) loss_err_body<EM_BINS>(A, betas, (int)blockIdx.x - n_stage);
    else transpose_in_body(G, (int)blockIdx.x);
}
// EM_ASYM: p = s(e)^beta_d; ML only, so there is no want_pow.
__global__ __launch_bounds__(256) void k_loss_err_asym(LossErrArgs A, const float *__restrict__ betas,
                                                       const float *__restrict__ kappas, int n_loss, StageArgs G) {
    const int n_stage = (int)gridDim.x - n_loss;
    if ((int)blockIdx.x < n_stage) {
        transpose_in_body(G, (int)blockIdx.x);
        return;
    }
    const int bid = (int)blockIdx.x - n_stage;
    const float *__restrict__ slab = A.slab, *__restrict__ bias = A.bias, *__restrict__ targ = A.targ;
    float *__restrict__ outT = A.outT, *__restrict__ eT = A.eT, *__restrict__ pT = A.pT;
    const int *__restrict__ first = A.first;
    const int dt = bid / A.b_tiles, bt = bid % A.b_tiles;
    const int d = dt * LOSS_DT + (int)(threadIdx.x >> 5), b = bt * 32 + (int)(threadIdx.x & 31);
    const size_t o = (size_t)d * A.Bp + b;
    float x = slab_sum(slab, o, (size_t)A.Dp * A.Bp, A.S);
    x = x + bias[d];
    float e = 0.0f, p = 0.0f;
    if (b < A.B && d < A.D) {
        e = x - targ[(size_t)(first ? first[b] + A.toff : b) * A.D + d];  // kernerror
        p = pow_or_self(asym_rule::skewed(e, kappas[d]), betas[d]);      // s(e) in the place of |e|, then kernindex2
    } else {
        x = 0.0f;
    }
    outT[o] = x;
    eT[o] = e;
    pT[o] = p;
}

// Per-dimension sum over the minibatch of |e|^beta in the reference's order (kernSumcol,
// DevFunc.cu:167-185 <- BP_GPU.cu:416: one thread per column, rows added sequentially).
// Used by k_loss_grad when it sums its own columns (one device, MLGGD_LOSS_FUSE=0; DT = 8).
// rows: LDS [DT][Bp+1]; must be called by all 256 threads.
template <int DT>
__device__ __forceinline__ void colsum_tile(const float *__restrict__ pT, int d0, int B, int Bp, float *rows,
                                            float *sums) {
    const int total = DT * Bp;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int dl = idx / Bp, b = idx - dl * Bp;
        rows[dl * (Bp + 1) + b] = pT[(size_t)(d0 + dl) * Bp + b];
    }
    __syncthreads();
    if (threadIdx.x < DT) {
        const float *col = rows + threadIdx.x * (Bp + 1);
        float s = col[0];  // kernSumcol: (*top) = (*fromp); then += in row order
        int b = 1;
        for (; b + 16 <= B; b += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) v[u] = col[b + u];
#pragma unroll
            for (int u = 0; u < 16; u++) s += v[u];
        }
        for (; b < B; b++) s += col[b];
        sums[threadIdx.x] = s;
    }
    __syncthreads();
}

// Data-parallel path only: this rank's share of the per-dimension sum of |e|^beta, summed over the ranks by an
// all-reduce right after -- so kernSumcol's sequential frame order (DevFunc.cu:167-185) cannot be kept anyway (the
// parity definition of the data-parallel step is "the single-device step up to summation order"), and the
// local part is a WAVEFRONT reduction (north_star): pT is [unit][frame] with the frames contiguous, so a wave reads a
// dimension's frames as coalesced 256-byte rows (lane = frame), each lane adds its frames b = lane, lane + 64, ...,
// and six cross-lane steps (DPP / ds_swizzle shuffles) finish the sum; 4 waves x 8 dimensions per workgroup, no LDS.
// On ONE device the statistic stays in kernSumcol's order (k_loss_ml, colsum_tile).
__global__ __launch_bounds__(256) void k_colsum(const float *__restrict__ pT, int B, int Bp,
                                                float *__restrict__ colsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int d = blockIdx.x * 32 + wave * 8 + q;
        const float *row = pT + (size_t)d * Bp;
        float s = 0.0f;
        for (int b = lane; b < B; b += 64) s += row[b];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) colsum[d] = s;
    }
}

// ---------------------------------------------------------------------------------------
// Output-layer loss, phase B: the gradient.  MLflag != 1: beta-norm gradient
// (kernSubClean2 + kernVecMulNum, DevFunc.cu:376-398,287-293 <- BP_GPU.cu:408-409).
// MLflag == 1: alpha_d = (beta * colsum_d / n)^(1/beta) (kernDivide, kernVecMulNum,
// kernindex2 <- BP_GPU.cu:417-420), g = sgn(e)|e|^(beta-1) * beta / alpha^beta / n
// (kernfunc2 + kernVecMulNum, DevFunc.cu:468-489 <- BP_GPU.cu:422-423).
// colsum_in == nullptr: the workgroup sums its 8 columns of pT itself (single GPU);
// otherwise colsum_in is the GLOBAL minibatch sum (all-reduced).  nf = global minibatch size.
// One workgroup per 8(d) x 32(b) tile; writes dEdXt and dEdX.  Dynamic LDS: 8*(Bp+1)+8 floats.
// ---------------------------------------------------------------------------------------
// The learned scale (mlggd_set_scale_mode, scale_rule.h): the _learn kernels' extra argument.  in / out are the two copies
// [alpha, v][Dp] of the engine's state: every launch of a step reads `in` and writes `out`, and the host swaps them once
// per step, so that workgroups sharing a column (b_tiles of them in the two-kernel form) and launches sharing a step
// (one per emulated rank) all see the same alpha, whichever of them has already written.
struct ScaleArgs {
    const float *in;
    float *out;
    float eta, mu, vmax;
};
// Column d < D with sum s: the rule's q, the denominator of this step's gradient; with write, (alpha', v') go to the
// other copy and alpha' to scalefactor.  The text of the rule is scale_rule.h's; pow_or_self and exp_det are evaluated here.
__device__ __forceinline__ float scale_learn_column(const ScaleArgs &S, int d, int Dp, float s, float nf, float beta,
                                                    bool write, float *__restrict__ scalefactor) {
    const float alpha = S.in[scale_rule::alpha_at(0, Dp, d)], v = S.in[scale_rule::velocity_at(0, Dp, d)];
    const float v2 = scale_rule::beta_s(s, nf, beta);  // kernDivide, kernVecMulNum
    float q, an, vn;
    if (scale_rule::seeds(alpha)) {
        an = pow_or_self(v2, 1.0f / beta);  // kernindex2 with ppp = 1.0f/shapefactor
        vn = 0.0f;
        q = pow_or_self(an, beta);
    } else {
        q = pow_or_self(alpha, beta);
        vn = scale_rule::velocity(v2, q, v, S.eta, S.mu, S.vmax);
        an = scale_rule::advance(alpha, exp_det(vn));
    }
    if (write) {
        S.out[scale_rule::alpha_at(0, Dp, d)] = an;
        S.out[scale_rule::velocity_at(0, Dp, d)] = vn;
        scalefactor[d] = an;
    }
    return q;
}
// beta and MLflag are read under EM_SHARED only: the other two models are ML by construction.  LEARN: the scale is the
// engine's state moved by scale_rule.h instead of the minibatch's closed form; every other statement is the same text.
template <int EM, bool LEARN = false>
__device__ __forceinline__ void loss_grad_body(const float *__restrict__ eT, const float *__restrict__ pT,
                                               const float *__restrict__ colsum_in, int B, int D, int Dp, int Bp,
                                               float beta_shared, const float *__restrict__ betas,
                                               const float *__restrict__ kappas, int MLflag, float nf, float inv_n,
                                               float *__restrict__ scalefactor, float *__restrict__ dEdXt,
                                               float *__restrict__ dEdX, int b_tiles, const ScaleArgs &S = ScaleArgs()) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ float denom[LOSS_DT];
    const bool ml = EM != EM_SHARED || MLflag == 1;
    const int dt = blockIdx.x / b_tiles, bt = blockIdx.x % b_tiles;
    const int d0 = dt * LOSS_DT;
    const int tid = threadIdx.x;
    if (ml) {
        float *rows = dyn, *sums = dyn + LOSS_DT * (Bp + 1);
        if (colsum_in == nullptr) {
            colsum_tile<LOSS_DT>(pT, d0, B, Bp, rows, sums);
        } else {
            if (tid < LOSS_DT) sums[tid] = colsum_in[d0 + tid];
            __syncthreads();
        }
        if (tid < LOSS_DT) {
            const int d = d0 + tid;
            float q = 1.0f;
            if (d < D) {
                const float beta = EM == EM_SHARED ? beta_shared : betas[d];
                if (LEARN) {
                    q = scale_learn_column(S, d, Dp, sums[tid], nf, beta, bt == 0, scalefactor);
                } else {
                    const float v1 = sums[tid] / nf;            // kernDivide
                    const float v2 = v1 * beta;                 // kernVecMulNum
                    const float alpha = pow_or_self(v2, 1.0f / beta);  // kernindex2 with ppp = 1.0f/shapefactor
                    if (bt == 0) scalefactor[d] = alpha;
                    q = pow_or_self(alpha, beta);                 // pow(vec[j], alpha) in kernfunc2
                }
            }
            denom[tid] = q;
        }
        __syncthreads();
    }
    const int dl = tid >> 5, d = d0 + dl, b = bt * 32 + (tid & 31);
    const size_t o = (size_t)d * Bp + b;
    const float e = eT[o];
    float g = 0.0f;
    if (b < B && d < D) {
        const float beta = EM == EM_SHARED ? beta_shared : betas[d];
        if (EM == EM_ASYM) {
            const float kappa = kappas[d];
            const float v = pow_or_self(asym_rule::skewed(e, kappa), beta - 1.0f) * beta / denom[dl];  // kernfunc2 at s(e)
            g = asym_rule::grad(e, v, kappa);
        } else if (ml) {
            if (e > 0) g = pow_or_self(e, beta - 1.0f) * beta / denom[dl];
            else if (e == 0) g = 0;
            else g = -pow_or_self(-e, beta - 1.0f) * beta / denom[dl];
        } else {
            if (e > 0) g = beta * pow_or_self(e, beta - 1);
            else if (e == 0) g = 0;
            else g = -beta * pow_or_self(-e, beta - 1);
        }
        g = g * inv_n;
    }
    dEdXt[o] = g;
    dEdX[(size_t)b * Dp + d] = g;
}
__global__ __launch_bounds__(256) void k_loss_grad(const float *__restrict__ eT, const float *__restrict__ pT,
                                                   const float *__restrict__ colsum_in, int B, int D, int Dp, int Bp,
                                                   float beta, int MLflag, float nf, float inv_n,
                                                   float *__restrict__ scalefactor, float *__restrict__ dEdXt,
                                                   float *__restrict__ dEdX, int b_tiles) {
    loss_grad_body<EM_SHARED>(eT, pT, colsum_in, B, D, Dp, Bp, beta, nullptr, nullptr, MLflag, nf, inv_n, scalefactor,
                              dEdXt, dEdX, b_tiles);
}
__global__ __launch_bounds__(256) void k_loss_grad_bins(const float *__restrict__ eT, const float *__restrict__ pT,
                                                        const float *__restrict__ colsum_in, int B, int D, int Dp,
                                                        int Bp, const float *__restrict__ betas, float nf, float inv_n,
                                                        float *__restrict__ scalefactor, float *__restrict__ dEdXt,
                                                        float *__restrict__ dEdX, int b_tiles) {
    loss_grad_body<EM_BINS>(eT, pT, colsum_in, B, D, Dp, Bp, 0.0f, betas, nullptr, 1, nf, inv_n, scalefactor, dEdXt, dEdX,
                            b_tiles);
}
__global__ __launch_bounds__(256) void k_loss_grad_asym(const float *__restrict__ eT, const float *__restrict__ pT,
                                                        const float *__restrict__ colsum_in, int B, int D, int Dp,
                                                        int Bp, const float *__restrict__ betas,
                                                        const float *__restrict__ kappas, float nf, float inv_n,
                                                        float *__restrict__ scalefactor, float *__restrict__ dEdXt,
                                                        float *__restrict__ dEdX, int b_tiles) {
    loss_grad_body<EM_ASYM>(eT, pT, colsum_in, B, D, Dp, Bp, 0.0f, betas, kappas, 1, nf, inv_n, scalefactor, dEdXt, dEdX,
                            b_tiles);
}
// The learned scale: ML only, so k_loss_grad_learn has no MLflag.
__global__ __launch_bounds__(256) void k_loss_grad_learn(const float *__restrict__ eT, const float *__restrict__ pT,
                                                         const float *__restrict__ colsum_in, int B, int D, int Dp,
                                                         int Bp, float beta, float nf, float inv_n,
                                                         float *__restrict__ scalefactor, float *__restrict__ dEdXt,
                                                         float *__restrict__ dEdX, int b_tiles, ScaleArgs S) {
    loss_grad_body<EM_SHARED, true>(eT, pT, colsum_in, B, D, Dp, Bp, beta, nullptr, nullptr, 1, nf, inv_n, scalefactor,
                                    dEdXt, dEdX, b_tiles, S);
}
__global__ __launch_bounds__(256) void k_loss_grad_learn_bins(const float *__restrict__ eT, const float *__restrict__ pT,
                                                              const float *__restrict__ colsum_in, int B, int D, int Dp,
                                                              int Bp, const float *__restrict__ betas, float nf,
                                                              float inv_n, float *__restrict__ scalefactor,
                                                              float *__restrict__ dEdXt, float *__restrict__ dEdX,
                                                              int b_tiles, ScaleArgs S) {
    loss_grad_body<EM_BINS, true>(eT, pT, colsum_in, B, D, Dp, Bp, 0.0f, betas, nullptr, 1, nf, inv_n, scalefactor, dEdXt,
                                  dEdX, b_tiles, S);
}
__global__ __launch_bounds__(256) void k_loss_grad_learn_asym(const float *__restrict__ eT, const float *__restrict__ pT,
                                                              const float *__restrict__ colsum_in, int B, int D, int Dp,
                                                              int Bp, const float *__restrict__ betas,
                                                              const float *__restrict__ kappas, float nf, float inv_n,
                                                              float *__restrict__ scalefactor, float *__restrict__ dEdXt,
                                                              float *__restrict__ dEdX, int b_tiles, ScaleArgs S) {
    loss_grad_body<EM_ASYM, true>(eT, pT, colsum_in, B, D, Dp, Bp, 0.0f, betas, kappas, 1, nf, inv_n, scalefactor, dEdXt,
                                  dEdX, b_tiles, S);
}

// MLflag != 1 needs no statistic over the minibatch, so phases A and B collapse into one
// elementwise pass: slab sum + bias -> error -> beta-norm gradient (same expressions and order as
// k_loss_err / k_loss_grad), written as dEdXt and dEdX.
struct LossNormArgs {
    const float *slab;
    int S;
    const float *bias, *targ;
    int B, D, Dp, Bp;
    float beta, inv_n;
    float *outT, *eT, *dEdXt, *dEdX;
    int b_tiles;
    const int *first;
    int toff;
};
__device__ __forceinline__ void loss_norm_body(const LossNormArgs &A, const int bid) {
    const float *__restrict__ slab = A.slab, *__restrict__ bias = A.bias, *__restrict__ targ = A.targ;
    float *__restrict__ outT = A.outT, *__restrict__ eT = A.eT, *__restrict__ dEdXt = A.dEdXt, *__restrict__ dEdX = A.dEdX;
    const int *__restrict__ first = A.first;
    const float beta = A.beta;
    const int dt = bid / A.b_tiles, bt = bid % A.b_tiles;
    const int d = dt * LOSS_DT + (int)(threadIdx.x >> 5), b = bt * 32 + (int)(threadIdx.x & 31);
    const size_t o = (size_t)d * A.Bp + b;
    float x = slab_sum(slab, o, (size_t)A.Dp * A.Bp, A.S);
    x = x + bias[d];
    float e = 0.0f, g = 0.0f;
    if (b < A.B && d < A.D) {
        e = x - targ[(size_t)(first ? first[b] + A.toff : b) * A.D + d];  // kernerror
        if (e > 0) g = beta * pow_or_self(e, beta - 1);                    // kernSubClean2
        else if (e == 0) g = 0;
        else g = -beta * pow_or_self(-e, beta - 1);
        g = g * A.inv_n;                                                   // kernVecMulNum
    } else {
        x = 0.0f;
    }
    outT[o] = x;
    eT[o] = e;
    dEdXt[o] = g;
    dEdX[(size_t)b * A.Dp + d] = g;
}
__global__ __launch_bounds__(256) void k_loss_norm(LossNormArgs A, int n_loss, StageArgs G) {
    const int n_stage = (int)gridDim.x - n_loss;  // staging blocks first: they are the longer ones
    if ((int)blockIdx.x >= n_stage) loss_norm_body(A, (int)blockIdx.x - n_stage);
    else transpose_in_body(G, (int)blockIdx.x);
}

// ---------------------------------------------------------------------------------------
// The whole ML-GGD loss (BP_GPU.cu:413-423: kernerror, kernabsolutevalus, kernindex2, kernSumcol, kernDivide,
// kernVecMulNum, kernindex2, kernfunc2, kernVecMulNum) in ONE launch on a single device: a workgroup of 1024
// threads owns 8 output units over ALL frames of the minibatch, so the per-dimension statistic never leaves its
// LDS: e and p = |e|^beta for its 8 x Bp elements (one per thread at B = 128), the 8 column sums in the reference's
// sequential order (8 threads, as kernSumcol), alpha and alpha^beta, then the gradient of the same elements.
// Replaces k_loss_err + k_loss_grad and the pT / eT round trip between them (ML step -3.5 us); the data-parallel
// path keeps the two-kernel form because the statistic has to be summed over the ranks in between.
// Dynamic LDS: 2 * 8 * (Bp + 1) floats.  The staging blocks of the next minibatch ride along as in k_loss_norm,
// four 256-thread tiles per 1024-thread workgroup.
// ---------------------------------------------------------------------------------------
struct LossMlArgs {
    const float *slab;
    int S;
    const float *bias, *targ;
    int B, D, Dp, Bp;
    float beta, nf, inv_n;
    float *outT, *eT, *scalefactor, *dEdXt, *dEdX;
    const int *first;
    int toff;
};
// wg: the loss workgroup, staging blocks not counted
template <int EM, bool LEARN = false>
__device__ __forceinline__ void loss_ml_body(const LossMlArgs &A, const float *__restrict__ betas,
                                             const float *__restrict__ kappas, const int wg,
                                             const ScaleArgs &S = ScaleArgs()) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ float denom[LOSS_DT];
    const float *__restrict__ slab = A.slab, *__restrict__ bias = A.bias, *__restrict__ targ = A.targ;
    const int *__restrict__ first = A.first;
    const int B = A.B, D = A.D, Dp = A.Dp, Bp = A.Bp;
    float *es = dyn, *ps = dyn + LOSS_DT * (Bp + 1);  // [8][Bp+1] each
    const int d0 = wg * LOSS_DT;
    const int tid = threadIdx.x, dl = tid >> 7, d = d0 + dl;  // 8 units x 128 frames per pass
    // uniform over the unit's 128 threads, two whole waves: pow_or_self's branches stay wave-uniform
    const float beta = EM == EM_SHARED ? A.beta : betas[d], kappa = EM == EM_ASYM ? kappas[d] : 1.0f;
    for (int b = tid & 127; b < Bp; b += 128) {
        const size_t o = (size_t)d * Bp + b;
        float x = slab_sum(slab, o, (size_t)Dp * Bp, A.S);
        x = x + bias[d];
        float e = 0.0f, p = 0.0f;
        if (b < B && d < D) {
            e = x - targ[(size_t)(first ? first[b] + A.toff : b) * D + d];  // kernerror
            p = pow_or_self(EM == EM_ASYM ? asym_rule::skewed(e, kappa) : fabsf(e), beta);  // kernabsolutevalus + kernindex2
        } else {
            x = 0.0f;
        }
        A.outT[o] = x;
        A.eT[o] = e;
        es[dl * (Bp + 1) + b] = e;
        ps[dl * (Bp + 1) + b] = p;
    }
    __syncthreads();
    if (tid < LOSS_DT) {
        const float *col = ps + tid * (Bp + 1);
        float s = col[0];  // kernSumcol: (*top) = (*fromp); then += in row order
        int b = 1;
        for (; b + 16 <= B; b += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) v[u] = col[b + u];
#pragma unroll
            for (int u = 0; u < 16; u++) s += v[u];
        }
        for (; b < B; b++) s += col[b];
        float q = 1.0f;
        if (d0 + tid < D) {
            const float beta = EM == EM_SHARED ? A.beta : betas[d0 + tid];  // the column this thread sums, not the unit of its passes
            if (LEARN) {
                q = scale_learn_column(S, d0 + tid, Dp, s, A.nf, beta, true, A.scalefactor);
            } else {
                const float v1 = s / A.nf;                  // kernDivide
                const float v2 = v1 * beta;                 // kernVecMulNum
                const float alpha = pow_or_self(v2, 1.0f / beta);  // kernindex2 with ppp = 1.0f/shapefactor
                A.scalefactor[d0 + tid] = alpha;
                q = pow_or_self(alpha, beta);                 // pow(vec[j], alpha) in kernfunc2
            }
        }
        denom[tid] = q;
    }
    __syncthreads();
    for (int b = tid & 127; b < Bp; b += 128) {
        const float e = es[dl * (Bp + 1) + b];
        float g = 0.0f;
        if (b < B && d < D) {
            if (EM == EM_ASYM) {
                const float v = pow_or_self(asym_rule::skewed(e, kappa), beta - 1.0f) * beta / denom[dl];
                g = asym_rule::grad(e, v, kappa);
            } else {
                if (e > 0) g = pow_or_self(e, beta - 1.0f) * beta / denom[dl];
                else if (e == 0) g = 0;
                else g = -pow_or_self(-e, beta - 1.0f) * beta / denom[dl];
            }
            g = g * A.inv_n;                                                  // kernVecMulNum
        }
        A.dEdXt[(size_t)d * Bp + b] = g;
        es[dl * (Bp + 1) + b] = g;  // this thread's own element: the row layout leaves below, 16 bytes at a time
    }
    // dEdX [frame][unit]: a frame's 8 units of this workgroup are 32 contiguous bytes -- two 16-byte stores per frame
    // (2 * Bp per workgroup) instead of eight 4-byte stores each into a line of its own (8 * Bp)
    __syncthreads();
    for (int t = tid; t < 2 * Bp; t += 1024) {
        const int b = t >> 1, h4 = (t & 1) * 4;
        float4 v;
        v.x = es[(h4 + 0) * (Bp + 1) + b];
        v.y = es[(h4 + 1) * (Bp + 1) + b];
        v.z = es[(h4 + 2) * (Bp + 1) + b];
        v.w = es[(h4 + 3) * (Bp + 1) + b];
        *reinterpret_cast<float4 *>(&A.dEdX[(size_t)b * Dp + d0 + h4]) = v;
    }
}
__global__ __launch_bounds__(1024) void k_loss_ml(LossMlArgs A, int n_loss, StageArgs G, int n_stage_tiles) {
    const int n_stage = (int)gridDim.x - n_loss;
    if ((int)blockIdx.x < n_stage) {
        transpose_in_body<4>(G, (int)blockIdx.x, n_stage_tiles);
        return;
    }
    loss_ml_body<EM_SHARED>(A, nullptr, nullptr, (int)blockIdx.x - n_stage);
}
__global__ __launch_bounds__(1024) void k_loss_ml_bins(LossMlArgs A, const float *__restrict__ betas, int n_loss,
                                                       StageArgs G, int n_stage_tiles) {
    const int n_stage = (int)gridDim.x - n_loss;
    if ((int)blockIdx.x < n_stage) {
        transpose_in_body<4>(G, (int)blockIdx.x, n_stage_tiles);
        return;
    }
    loss_ml_body<EM_BINS>(A, betas, nullptr, (int)blockIdx.x - n_stage);
}
__global__ __launch_bounds__(1024) void k_loss_ml_asym(LossMlArgs A, const float *__restrict__ betas,
                                                       const float *__restrict__ kappas, int n_loss, StageArgs G,
                                                       int n_stage_tiles) {
    const int n_stage = (int)gridDim.x - n_loss;
    if ((int)blockIdx.x < n_stage) {
        transpose_in_body<4>(G, (int)blockIdx.x, n_stage_tiles);
        return;
    }
    loss_ml_body<EM_ASYM>(A, betas, kappas, (int)blockIdx.x - n_stage);
}
__global__ __launch_bounds__(1024) void k_loss_ml_learn(LossMlArgs A, ScaleArgs S, int n_loss, StageArgs G,
                                                        int n_stage_tiles) {
    const int n_stage = (int)gridDim.x - n_loss;
    if ((int)blockIdx.x < n_stage) {
        transpose_in_body<4>(G, (int)blockIdx.x, n_stage_tiles);
        return;
    }
    loss_ml_body<EM_SHARED, true>(A, nullptr, nullptr, (int)blockIdx.x - n_stage, S);
}
__global__ __launch_bounds__(1024) void k_loss_ml_learn_bins(LossMlArgs A, ScaleArgs S, const float *__restrict__ betas,
                                                             int n_loss, StageArgs G, int n_stage_tiles) {
    const int n_stage = (int)gridDim.x - n_loss;
    if ((int)blockIdx.x < n_stage) {
        transpose_in_body<4>(G, (int)blockIdx.x, n_stage_tiles);
        return;
    }
    loss_ml_body<EM_BINS, true>(A, betas, nullptr, (int)blockIdx.x - n_stage, S);
}
__global__ __launch_bounds__(1024) void k_loss_ml_learn_asym(LossMlArgs A, ScaleArgs S, const float *__restrict__ betas,
                                                             const float *__restrict__ kappas, int n_loss, StageArgs G,
                                                             int n_stage_tiles) {
    const int n_stage = (int)gridDim.x - n_loss;
    if ((int)blockIdx.x < n_stage) {
        transpose_in_body<4>(G, (int)blockIdx.x, n_stage_tiles);
        return;
    }
    loss_ml_body<EM_ASYM, true>(A, betas, kappas, (int)blockIdx.x - n_stage, S);
}

// Forward-only output (cv_bunch_single, BP_GPU.cu:442-512): out[b][d] = bias + sum_s slab,
// compact row-major [B][D] for the D2H copy.
__global__ __launch_bounds__(256) void k_out_rowmajor(const float *__restrict__ slab, int S,
                                                      const float *__restrict__ bias, int B, int D, int Dp, int Bp,
                                                      float *__restrict__ out, int b_tiles) {
    __shared__ float t[32][33];
    const int dt = blockIdx.x / b_tiles, bt = blockIdx.x % b_tiles;
    const int d0 = dt * 32, b0 = bt * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int d = d0 + ty + 8 * q;
        const size_t o = (size_t)d * Bp + b0 + tx;
        const float x = slab_sum(slab, o, (size_t)Dp * Bp, S);
        t[ty + 8 * q][tx] = x + bias[d];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int b = b0 + ty + 8 * q, d = d0 + tx;
        if (b < B && d < D) out[(size_t)b * D + d] = t[tx][ty + 8 * q];
    }
}

// ---------------------------------------------------------------------------------------
// CV metrics reduced on the device: per 32(d) x 32(b) tile of one CV bunch the three sums
// that CrossValid / CrossValiddB / CrossValid2 accumulate on the host (BP_GPU.cu:207-213, 240-250, 293-298):
//   sum (o-t)^2,   sum |o-t|,   sum (|t-o| / alpha_d)^beta
// Every term is formed in fp32 exactly as the host loops form it; the SUMS are kept in double (a tree over
// the tile, one double triple per tile, tiles and bunches combined on the host in double), so this path does
// not reproduce the reference's fp32 frame-major accumulation order -- the host-order path stays the default
// for the log lines.  Nothing of size n x D leaves the device.
// ---------------------------------------------------------------------------------------
struct CvArgs {
    const float *slab;
    int S;
    const float *bias, *targ;
    int B, D, Dp, Bp;
    float beta;
    const float *alpha;  // scalefactor [D]; nullptr: no likelihood term
    const int *first;
    int toff, b_tiles;
    double *partial;     // [tiles][3] of this bunch
};
// The models differ in the likelihood term only (A.beta is read under EM_SHARED alone): |t - o| / alpha_d, under
// EM_ASYM s(o - t) / alpha_d; the two shape-free sums are the same statements.
template <int EM>
__device__ __forceinline__ void cv_reduce_body(const CvArgs A, const float *__restrict__ betas,
                                               const float *__restrict__ kappas) {
    __shared__ float tt[32][33];
    __shared__ double red[4][3];
    const int dt = blockIdx.x / A.b_tiles, bt = blockIdx.x % A.b_tiles;
    const int d0 = dt * 32, b0 = bt * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int b = b0 + ty + 8 * q, d = d0 + tx;
        tt[ty + 8 * q][tx] = (b < A.B && d < A.D) ? A.targ[(size_t)(A.first ? A.first[b] + A.toff : b) * A.D + d] : 0.0f;
    }
    __syncthreads();
    double sq = 0.0, ab = 0.0, ll = 0.0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int dl = ty + 8 * q, d = d0 + dl, b = b0 + tx;
        if (b < A.B && d < A.D) {
            float x = slab_sum(A.slab, (size_t)d * A.Bp + b, (size_t)A.Dp * A.Bp, A.S);
            x = x + A.bias[d];
            const float t = tt[tx][dl];
            sq += (double)((x - t) * (x - t));   // BP_GPU.cu:211
            ab += (double)fabsf(x - t);           // BP_GPU.cu:246
            if (A.alpha)                          // BP_GPU.cu:295-296
                ll += (double)pow_or_self((EM == EM_ASYM ? asym_rule::skewed(x - t, kappas[d]) : fabsf(t - x)) / A.alpha[d],
                                          EM == EM_SHARED ? A.beta : betas[d]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sq += __shfl_down(sq, off, 64);
        ab += __shfl_down(ab, off, 64);
        ll += __shfl_down(ll, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave][0] = sq;
        red[wave][1] = ab;
        red[wave][2] = ll;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int j = threadIdx.x;
        A.partial[(size_t)blockIdx.x * 3 + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
    }
}
__global__ __launch_bounds__(256) void k_cv_reduce(CvArgs A) { cv_reduce_body<EM_SHARED>(A, nullptr, nullptr); }
__global__ __launch_bounds__(256) void k_cv_reduce_bins(CvArgs A, const float *__restrict__ betas) {
    cv_reduce_body<EM_BINS>(A, betas, nullptr);
}
__global__ __launch_bounds__(256) void k_cv_reduce_asym(CvArgs A, const float *__restrict__ betas,
                                                        const float *__restrict__ kappas) {
    cv_reduce_body<EM_ASYM>(A, betas, kappas);
}

// Dropout on the transposed activations (kernDropout, DevFunc.cu:26-34 <- BP_GPU.cu:344-355):
// zero where uniform < p, no rescale.  The reference draws from cuRAND's default generator;
// this engine uses a counter-based hash (documented deviation: streams cannot be matched).
__device__ __forceinline__ unsigned mix32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__global__ __launch_bounds__(256) void k_dropout(float *__restrict__ Yt, float *__restrict__ Yrow, int units,
                                                 int unitsp, int ldrow, int B, int Bp, float p, unsigned seed,
                                                 unsigned step) {
    const size_t n = (size_t)unitsp * Bp;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int u = (int)(idx / Bp), b = (int)(idx % Bp);
    if (u >= units || b >= B) return;
    const unsigned hsh = mix32(mix32(seed ^ (step * 0x9e3779b9u)) ^ (unsigned)idx);
    const float r = (float)(hsh >> 8) * (1.0f / 16777216.0f);
    if (r < p) {
        Yt[idx] = 0.0f;
        if (Yrow) Yrow[(size_t)b * ldrow + u] = 0.0f;
    }
}

// kernWeightMultiP (DevFunc.cu:19-25 <- BP_GPU.cu:484-501): CV-time weight scaling.
__global__ __launch_bounds__(256) void k_scale(float *__restrict__ x, size_t n, float p) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) x[idx] = x[idx] * p;
}
