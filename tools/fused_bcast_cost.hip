// tools/fused_bcast_cost.hip -- gfx950 microbenchmark behind profiles/riccati_fused_broadcast_ab.jsonl: what does a row broadcast that feeds ONE
// FP64 multiply-add cost a wave, and the wave that shares its SIMD, as the pair the compiler emits and as the fused DPP form it never emits?
//   pair        v_mov_b64_dpp tmp, src row_newbcast  +  v_fma_f64 acc, tmp, y, acc          (bcast16 + fma of csrc/tmpc_riccati.hpp)
//   nop_fused   s_nop 1  +  v_fmac_f64_dpp acc, src, y row_newbcast                         (the wait states a DPP read needs after a VALU write of src)
//   fused       v_fmac_f64_dpp acc, src, y row_newbcast, src written by no VALU instruction of the loop
//   fma         v_fma_f64 acc, src, y, acc: no broadcast at all (the floor)
// Each as K = 8 INDEPENDENT accumulators and as ONE dependent accumulation chain (K = 1), with EXEC = lanes 0..7 (the useful lanes of a Riccati row) and
// with all 64 lanes (what the stage loops run with), one wave per SIMD and two.  A test is a loop of ITER x 16 unrolled repetitions, the 16 in one
// asm statement (the compiler neither pads nor re-orders inside one); cycles = s_memtime deltas of the slowest wave, as tools/chain_floor.hip.
// grid = 1 workgroup of 64 x 4 x W threads: W waves on each of the four SIMDs of one CU.  One JSON line per test on stdout.
// Second part, behind profiles/forward_sweep_fused_sum_ab.jsonl: the forward sweep's two column sums of a stage (lane 0 of a 16-lane row adds lanes 2..6 of
// pa to its s, lane 8 lanes 10..14, each in the order m = 0..4) in four forms, written as a stage of riccati_sweeps_rows would have them and left to the compiler:
//   shl_add     five times (two v_mov_b32_dpp row_shl:(2 + m) bound_ctrl:0  +  v_add_f64)                       (dpp_shift_zero + add: what the kernels have)
//   fused_two   s_nop 1  +  five v_fmac_f64_dpp s0, pa, 1.0 row_newbcast:(2 + m)  interleaved with five  s1, pa, 1.0 row_newbcast:(10 + m)
//   fused_copy  the same ten behind two v_mov_b64 that copy the accumulators' start values instead of the pad: the copies a caller needs whose start value
//               stays live are the two wait states.  (Both two-accumulator forms were built into the kernels: the same bits, 4.0 k VALU instructions per
//               solve fewer, and no gain on the bench launch -- the record says why; the kernels keep shl_add.)
//   fused_mask  s_nop 1  +  five v_fmac_f64_dpp s, pa, 1.0 row_newbcast:(2 + m) bank_mask:0x3  +  five row_newbcast:(10 + m) bank_mask:0xc: ONE accumulator,
//               each chain on its half of the row.  It assembles and it is WRONG on gfx950: lanes 0 and 8 do not end with the sums of the other two forms
//               (an instruction that follows one with another bank mask reads a stale accumulator); kept here as the evidence, not used by any kernel.
// pa = a0 x is multiplied anew in front of every sum (the pad is needed), ordered behind the previous sum but not computed from it, so lanes 0 and 8 must
// end with the same bits in every form.  As ONE dependent chain of sums and as K = 4 independent ones, 64 lanes, one wave per SIMD and two; cycles per sum
// (the register copies a caller needs whose start value stays live -- none for shl_add, two for fused_two, one for fused_mask -- are in fused_copy only).
// Build: hipcc --offload-arch=gfx950 -O3 -o fused_bcast_cost fused_bcast_cost.hip        Run: ./fused_bcast_cost [iters]   (about a second)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

enum Form { F_PAIR = 0, F_NOP_FUSED, F_FUSED, F_FMA, F_COUNT };
static const char *kForm[F_COUNT] = {"pair: v_mov_b64_dpp + v_fma_f64", "nop_fused: s_nop 1 + v_fmac_f64_dpp", "fused: v_fmac_f64_dpp, source not written", "fma: v_fma_f64, no broadcast"};

#define DPPC " row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
// one multiply-add of each form: A = accumulator, S = source of the broadcast, T = temporary of the pair, %[y] the other multiplicand
#define MA_PAIR(A, S, T) "v_mov_b64_dpp " T ", " S DPPC "v_fma_f64 " A ", " T ", %[y], " A "\n\t"
#define MA_NOPF(A, S, T) "s_nop 1\n\tv_fmac_f64_dpp " A ", " S ", %[y]" DPPC
#define MA_FUSE(A, S, T) "v_fmac_f64_dpp " A ", " S ", %[y]" DPPC
#define MA_FMA(A, S, T) "v_fma_f64 " A ", " S ", %[y], " A "\n\t"
// eight independent accumulators / eight links of one chain (two temporaries in turn, as a register allocator would)
#define IND8(M) M("%[a0]", "%[s0]", "%[t0]") M("%[a1]", "%[s1]", "%[t1]") M("%[a2]", "%[s2]", "%[t2]") M("%[a3]", "%[s3]", "%[t3]") \
                M("%[a4]", "%[s4]", "%[t4]") M("%[a5]", "%[s5]", "%[t5]") M("%[a6]", "%[s6]", "%[t6]") M("%[a7]", "%[s7]", "%[t7]")
#define DEP8(M) M("%[a0]", "%[s0]", "%[t0]") M("%[a0]", "%[s1]", "%[t1]") M("%[a0]", "%[s2]", "%[t0]") M("%[a0]", "%[s3]", "%[t1]") \
                M("%[a0]", "%[s4]", "%[t0]") M("%[a0]", "%[s5]", "%[t1]") M("%[a0]", "%[s6]", "%[t0]") M("%[a0]", "%[s7]", "%[t1]")
#define OPERANDS : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [a3] "+v"(a[3]), [a4] "+v"(a[4]), [a5] "+v"(a[5]), [a6] "+v"(a[6]), [a7] "+v"(a[7]), \
                   [t0] "+v"(t[0]), [t1] "+v"(t[1]), [t2] "+v"(t[2]), [t3] "+v"(t[3]), [t4] "+v"(t[4]), [t5] "+v"(t[5]), [t6] "+v"(t[6]), [t7] "+v"(t[7]) \
                 : [s0] "v"(s[0]), [s1] "v"(s[1]), [s2] "v"(s[2]), [s3] "v"(s[3]), [s4] "v"(s[4]), [s5] "v"(s[5]), [s6] "v"(s[6]), [s7] "v"(s[7]), [y] "v"(y)

#define X16(B) B B B B B B B B B B B B B B B B
// 16 repetitions of 8 multiply-adds in ONE statement (between two statements the compiler pads an s_nop 0 of its own)
template <int FORM, bool DEP>
__device__ __forceinline__ void rep128(double (&a)[8], double (&t)[8], const double (&s)[8], double y)
{
    if constexpr (FORM == F_PAIR && !DEP) asm volatile(X16(IND8(MA_PAIR)) OPERANDS);
    else if constexpr (FORM == F_PAIR) asm volatile(X16(DEP8(MA_PAIR)) OPERANDS);
    else if constexpr (FORM == F_NOP_FUSED && !DEP) asm volatile(X16(IND8(MA_NOPF)) OPERANDS);
    else if constexpr (FORM == F_NOP_FUSED) asm volatile(X16(DEP8(MA_NOPF)) OPERANDS);
    else if constexpr (FORM == F_FUSED && !DEP) asm volatile(X16(IND8(MA_FUSE)) OPERANDS);
    else if constexpr (FORM == F_FUSED) asm volatile(X16(DEP8(MA_FUSE)) OPERANDS);
    else if constexpr (!DEP) asm volatile(X16(IND8(MA_FMA)) OPERANDS);
    else asm volatile(X16(DEP8(MA_FMA)) OPERANDS);
}

template <int FORM, bool DEP>
__global__ __launch_bounds__(512) void bench(double *out, long long *cyc, long long *rt, int iters, int active, double y, double seed)
{
    const int tid = threadIdx.x, lane = tid & 63;
    double a[8], s[8], t[8] = {};
#pragma unroll
    for (int c = 0; c < 8; c++) { a[c] = seed + 1e-3 * c; s[c] = 1.0 + 0.125 * c + 1e-3 * (lane & 15); }
    long long t0 = 0, t1 = 0, r0 = 0, r1 = 0;
    if (lane < active) {                                 // EXEC = lanes 0 .. active-1 of every wave for the whole timed region
        r0 = __builtin_amdgcn_s_memrealtime();
        t0 = __builtin_amdgcn_s_memtime();
        for (int it = 0; it < iters; it++) rep128<FORM, DEP>(a, t, s, y);
        double sum = 0.0;
#pragma unroll
        for (int c = 0; c < 8; c++) sum += a[c];
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::"v"(sum));
        t1 = __builtin_amdgcn_s_memtime();
        r1 = __builtin_amdgcn_s_memrealtime();
        out[tid] = sum;
    }
    if (lane == 0) { cyc[tid / 64] = t1 - t0; rt[tid / 64] = r1 - r0; }
}

struct Result { int form, dep, W, active; double cyc_per_ma, simd_cyc_per_ma, mhz, check; };

template <int FORM, bool DEP>
static Result run(int W, int active, int iters, double *d_out, long long *d_cyc, long long *d_rt)
{
    const int threads = 64 * 4 * W;
    std::vector<long long> cyc(4 * W), rt(4 * W);
    // y = 2^-30: the accumulators stay finite and far from 0 for any ITER a run can take
    for (int rep = 0; rep < 3; rep++) {
        hipLaunchKernelGGL((bench<FORM, DEP>), dim3(1), dim3(threads), 0, 0, d_out, d_cyc, d_rt, iters, active, 0x1p-30, 1.25);
        CHECK(hipDeviceSynchronize());
    }
    CHECK(hipMemcpy(cyc.data(), d_cyc, cyc.size() * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(rt.data(), d_rt, rt.size() * 8, hipMemcpyDeviceToHost));
    double chk = 0.0;
    CHECK(hipMemcpy(&chk, d_out + 3, 8, hipMemcpyDeviceToHost));          // lane 3 = the broadcast lane: the same sum for every form
    long long cmax = 0, rmax = 0;
    for (size_t i = 0; i < cyc.size(); i++) { if (cyc[i] > cmax) cmax = cyc[i]; if (rt[i] > rmax) rmax = rt[i]; }
    const double mas = (double)iters * 16 * 8;                             // multiply-adds of one wave
    Result r;
    r.form = FORM; r.dep = DEP; r.W = W; r.active = active; r.check = chk;
    r.cyc_per_ma = cmax / mas;                                             // what the wave waits for one multiply-add
    r.simd_cyc_per_ma = cmax / (mas * W);                                  // what one multiply-add takes of the SIMD both waves share
    r.mhz = rmax > 0 ? (double)cmax / (rmax * 10.0) * 1e3 : 0.0;           // s_memrealtime ticks at 100 MHz
    return r;
}

// ---- the forward sweep's column sums ----------------------------------------------------------------------------------------------------------
enum SumForm { S_SHL = 0, S_TWO, S_MASK, S_COPY, S_COUNT };
static const char *kSumForm[S_COUNT] = {"shl_add: 10 v_mov_b32_dpp row_shl + 5 v_add_f64", "fused_two: s_nop 1 + 2 x 5 v_fmac_f64_dpp on two accumulators",
                                        "fused_mask: s_nop 1 + 10 bank-masked v_fmac_f64_dpp on one accumulator (wrong sums)",
                                        "fused_copy: 2 v_mov_b64 + 2 x 5 v_fmac_f64_dpp on two accumulators, no pad"};

template <int CTRL>
__device__ __forceinline__ double shl_zero(double x)
{
    union { double d; int i[2]; } u, o;
    u.d = x;
    o.i[0] = __builtin_amdgcn_mov_dpp(u.i[0], CTRL, 0xf, 0xf, true);
    o.i[1] = __builtin_amdgcn_mov_dpp(u.i[1], CTRL, 0xf, 0xf, true);
    return o.d;
}
#define SUM_T(lane, banks) "v_fmac_f64_dpp %[s], %[pa], %[one] row_newbcast:" #lane " row_mask:0xf bank_mask:" #banks "\n\t"
#define SUM_2(acc, lane) "v_fmac_f64_dpp %[" #acc "], %[pa], %[one] row_newbcast:" #lane " row_mask:0xf bank_mask:0xf\n\t"
// (s1 is the second column's accumulator of fused_two; the other two forms keep both columns in s)
template <int FORM>
__device__ __forceinline__ void column_sums(double &s, double &s1, double pa, double one)
{
    if constexpr (FORM == S_SHL) {
        s += shl_zero<0x102>(pa); s += shl_zero<0x103>(pa); s += shl_zero<0x104>(pa); s += shl_zero<0x105>(pa); s += shl_zero<0x106>(pa);
    } else if constexpr (FORM == S_TWO)
        asm("s_nop 1\n\t" SUM_2(s0, 2) SUM_2(s1, 10) SUM_2(s0, 3) SUM_2(s1, 11) SUM_2(s0, 4) SUM_2(s1, 12) SUM_2(s0, 5) SUM_2(s1, 13) SUM_2(s0, 6) SUM_2(s1, 14)
            : [s0] "+&v"(s), [s1] "+&v"(s1) : [pa] "v"(pa), [one] "v"(one));
    else if constexpr (FORM == S_COPY) {
        double t0, t1;
        asm("v_mov_b64 %[s0], %[y0]\n\tv_mov_b64 %[s1], %[y1]\n\t"
            SUM_2(s0, 2) SUM_2(s1, 10) SUM_2(s0, 3) SUM_2(s1, 11) SUM_2(s0, 4) SUM_2(s1, 12) SUM_2(s0, 5) SUM_2(s1, 13) SUM_2(s0, 6) SUM_2(s1, 14)
            : [s0] "=&v"(t0), [s1] "=&v"(t1) : [y0] "v"(s), [y1] "v"(s1), [pa] "v"(pa), [one] "v"(one));
        s = t0; s1 = t1;
    } else
        asm("s_nop 1\n\t" SUM_T(2, 0x3) SUM_T(3, 0x3) SUM_T(4, 0x3) SUM_T(5, 0x3) SUM_T(6, 0x3) SUM_T(10, 0xc) SUM_T(11, 0xc) SUM_T(12, 0xc) SUM_T(13, 0xc) SUM_T(14, 0xc)
            : [s] "+&v"(s) : [pa] "v"(pa), [one] "v"(one));
}

template <int FORM, int K>
__global__ __launch_bounds__(512) void bench_sum(double *out, long long *cyc, long long *rt, int iters, double a0, double seed)
{
    const int tid = threadIdx.x, lane = tid & 63;
    double s[K], s1[K], x[K], one = 1.0;
    asm volatile("" : "+v"(one));
#pragma unroll
    for (int c = 0; c < K; c++) { s[c] = s1[c] = seed + 1e-3 * c; x[c] = 1.0 + 0.125 * c + 1e-3 * (lane & 15); }
    const long long r0 = __builtin_amdgcn_s_memrealtime(), t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int r = 0; r < 8; r++) {
#pragma unroll
            for (int c = 0; c < K; c++) {
                asm volatile("" : "+v"(x[c]) : "v"(s[c]));       // the product follows the chain's previous sum, without reading it
                column_sums<FORM>(s[c], s1[c], a0 * x[c], one);
            }
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < K; c++) sum += ((FORM == S_TWO || FORM == S_COPY) && (lane & 8)) ? s1[c] : s[c];      // (two accumulators: the upper half-row's sums are in s1)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::"v"(sum));
    const long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    out[tid] = sum;
    if (lane == 0) { cyc[tid / 64] = t1 - t0; rt[tid / 64] = r1 - r0; }
}

struct SumResult { int form, K, W; double cyc_per_sum, simd_cyc_per_sum, mhz, lane0, lane8; };

template <int FORM, int K>
static SumResult run_sum(int W, int iters, double *d_out, long long *d_cyc, long long *d_rt)
{
    const int threads = 64 * 4 * W;
    std::vector<long long> cyc(4 * W), rt(4 * W);
    for (int rep = 0; rep < 3; rep++) {
        hipLaunchKernelGGL((bench_sum<FORM, K>), dim3(1), dim3(threads), 0, 0, d_out, d_cyc, d_rt, iters, 0x1p-30, 1.25);
        CHECK(hipDeviceSynchronize());
    }
    CHECK(hipMemcpy(cyc.data(), d_cyc, cyc.size() * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(rt.data(), d_rt, rt.size() * 8, hipMemcpyDeviceToHost));
    double chk[9];
    CHECK(hipMemcpy(chk, d_out, sizeof chk, hipMemcpyDeviceToHost));       // lanes 0 and 8: the two column sums, the same bits in both forms
    long long cmax = 0, rmax = 0;
    for (size_t i = 0; i < cyc.size(); i++) { if (cyc[i] > cmax) cmax = cyc[i]; if (rt[i] > rmax) rmax = rt[i]; }
    const double sums = (double)iters * 8 * K;                             // stage sums (both columns) of one wave
    SumResult r;
    r.form = FORM; r.K = K; r.W = W; r.lane0 = chk[0]; r.lane8 = chk[8];
    r.cyc_per_sum = cmax / sums;
    r.simd_cyc_per_sum = cmax / (sums * W);
    r.mhz = rmax > 0 ? (double)cmax / (rmax * 10.0) * 1e3 : 0.0;
    return r;
}

int main(int argc, char **argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 4096;
    double *d_out; long long *d_cyc, *d_rt;
    CHECK(hipMalloc(&d_out, 512 * 8)); CHECK(hipMalloc(&d_cyc, 64 * 8)); CHECK(hipMalloc(&d_rt, 64 * 8));
    CHECK(hipMemset(d_out, 0, 512 * 8));
    std::vector<Result> res;
    for (int active = 8; active <= 64; active += 56)
        for (int W = 1; W <= 2; W++) {
            res.push_back(run<F_PAIR, false>(W, active, iters, d_out, d_cyc, d_rt));
            res.push_back(run<F_NOP_FUSED, false>(W, active, iters, d_out, d_cyc, d_rt));
            res.push_back(run<F_FUSED, false>(W, active, iters, d_out, d_cyc, d_rt));
            res.push_back(run<F_FMA, false>(W, active, iters, d_out, d_cyc, d_rt));
            res.push_back(run<F_PAIR, true>(W, active, iters, d_out, d_cyc, d_rt));
            res.push_back(run<F_NOP_FUSED, true>(W, active, iters, d_out, d_cyc, d_rt));
            res.push_back(run<F_FUSED, true>(W, active, iters, d_out, d_cyc, d_rt));
            res.push_back(run<F_FMA, true>(W, active, iters, d_out, d_cyc, d_rt));
        }
    hipDeviceProp_t p; CHECK(hipGetDeviceProperties(&p, 0));
    for (size_t i = 0; i < res.size(); i++) {
        const Result &r = res[i];
        printf("{\"what\": \"fused_bcast_cost\", \"device\": \"%s\", \"gcn_arch\": \"%s\", \"iters\": %d, \"form\": \"%s\", \"chain\": \"%s\", \"active_lanes\": %d, "
               "\"waves_per_simd\": %d, \"cycles_per_multiply_add_per_wave\": %.3f, \"simd_cycles_per_multiply_add\": %.3f, \"memtime_mhz\": %.1f, \"lane3_sum\": %.17g}\n",
               p.name, p.gcnArchName, iters, kForm[r.form], r.dep ? "dependent" : "independent", r.active, r.W, r.cyc_per_ma, r.simd_cyc_per_ma, r.mhz, r.check);
    }
    std::vector<SumResult> sres;
    for (int W = 1; W <= 2; W++) {
        sres.push_back(run_sum<S_SHL, 1>(W, iters, d_out, d_cyc, d_rt));
        sres.push_back(run_sum<S_TWO, 1>(W, iters, d_out, d_cyc, d_rt));
        sres.push_back(run_sum<S_MASK, 1>(W, iters, d_out, d_cyc, d_rt));
        sres.push_back(run_sum<S_COPY, 1>(W, iters, d_out, d_cyc, d_rt));
        sres.push_back(run_sum<S_SHL, 4>(W, iters, d_out, d_cyc, d_rt));
        sres.push_back(run_sum<S_TWO, 4>(W, iters, d_out, d_cyc, d_rt));
        sres.push_back(run_sum<S_MASK, 4>(W, iters, d_out, d_cyc, d_rt));
        sres.push_back(run_sum<S_COPY, 4>(W, iters, d_out, d_cyc, d_rt));
    }
    for (size_t i = 0; i < sres.size(); i++) {
        const SumResult &r = sres[i];
        printf("{\"what\": \"fwd_column_sum_cost\", \"device\": \"%s\", \"gcn_arch\": \"%s\", \"iters\": %d, \"form\": \"%s\", \"chain\": \"%s\", \"active_lanes\": 64, "
               "\"waves_per_simd\": %d, \"cycles_per_sum_per_wave\": %.3f, \"simd_cycles_per_sum\": %.3f, \"memtime_mhz\": %.1f, \"lane0_sum\": %.17g, \"lane8_sum\": %.17g}\n",
               p.name, p.gcnArchName, iters, kSumForm[r.form], r.K == 1 ? "dependent" : "4 independent", r.W, r.cyc_per_sum, r.simd_cyc_per_sum, r.mhz, r.lane0, r.lane8);
    }
    return 0;
}
