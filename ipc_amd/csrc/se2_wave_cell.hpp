// SE(2) cell solver, one WAVE (W = 1, chains up to 64 M poses) or a PAIR of waves (W = 2, up to
// 128 M poses) per cell.
//
// The block kernel (se2_cell.hpp) spreads one chain over W waves and pays a workgroup barrier
// plus an LDS round trip for every reduction / scan / neighbour hand-off, with one cell resident
// per CU.  Here:
//   * lane l owns the M CONSECUTIVE poses l*M+1 .. l*M+M (lane-major), so the chain neighbour
//     of a slot is the previous slot of the same lane (a register); only slot 0 takes one DPP
//     shift from the lane below.  Prefix sums are an in-lane serial pass + ONE wave scan,
//     reductions are in-lane accumulation + ONE wave reduction.  No workgroup barrier anywhere.
//   * the four waves of a workgroup (one per SIMD, up to 512 registers each) work on four
//     different cells (W = 1) or two (W = 2) and fetch the next one from a global counter when
//     done, so a CU always has independent dog-legs in flight.
//   * W = 2: the two waves of a cell exchange the boundary pose / force / step vectors, partial
//     sums and scan carries through a sequence-numbered, double-buffered LDS mailbox (PairBox).
//   * the chain constants of the residual pass (5 measurement + 6 information values per edge)
//     are staged ONCE per workgroup for the whole window of the launch, one record per edge, and
//     shared by every cell it solves; M is odd so the lane stride of M records is bank-conflict
//     free, and a slot's constants sit at compile-time offsets from one per-lane address.
//   * trial poses / trial errors are not stored in vector registers: a trial is one sweep that steps, evaluates and
//     sums chi2 on the fly.  An accepted trial is re-swept once to commit (same coefficients, same bits), or, in the
//     kept-trial variants (KEEP_TRIAL, the se2_*_kernel_kt kernels), read back from the accumulator registers where
//     the trial sweep parked its poses (and, for M <= 8, its errors) by hand.  For M > 8 the committed
//     errors are not stored across iterations either: each iteration recomputes them (M = 9, 11: once, in phase A,
//     and parks them in accumulator registers for phases B1 and C; M = 13: in each of the three phases).
//   * with one wave per SIMD every instruction costs issue time: the per-slot code is pinned in
//     place (IPC_PIN*), loop end points are found by one bit test per slot, constants are fetched
//     one slot ahead where registers allow.
// Mathematics, dog-leg control flow and shortcuts are those of se2_cell.hpp.
#pragma once
#include "se2_cell.hpp"

namespace ipc {

template <int NL>
struct WaveScratch {          // per cell (one wave, or a pair of waves), LDS
    LoopConst lc[NL];
    LoopState ls[2][NL];
    double lvec[NL][2][3];
    double red[4][32];        // wide reduction, one row per wave of the cell
};

// Mailbox of a wave pair that solves one cell together (W == 2).  The two waves run on different
// SIMDs of the same workgroup and execute the same sequence of exchanges; an exchange is "write
// my values, post my sequence number, wait for the partner's, read the partner's values", double
// buffered on the sequence parity.  LDS operations of one wave complete in order, so the data is
// visible before the flag.
//
// The payload is moved with RELAXED ATOMIC loads / stores (workgroup scope), not plain ones.  The instructions are the
// same ds_read / ds_write, but (i) the protocol is then race-free for every lane by the memory model -- with plain
// accesses only lane 0, which posts the flag, is ordered against the partner's next overwrite of the buffer; the other
// lanes' reads are ordered by the wave's lock-step execution, which the model knows nothing about -- and (ii) the
// compiler waits for a payload read where it is issued instead of leaving it in flight across the exec-mask juggling
// and the branches that follow.  With plain accesses the kernels whose errors are recomputed (M > 8) give wrong,
// run-to-run varying results when built with -mllvm -amdgpu-sched-strategy=max-ilp (round 4, DESIGN.md 7:
// tools/maxilp_repro.py; the read of the partner's chi2 partial sum in the trial sweep is the one that matters);
// with atomic accesses both scheduling strategies give bit-identical results.  -DIPC_MAILBOX_PLAIN restores the plain
// accesses for that reproducer.
struct PairBox {
    double data[4][2][8];     // [wave of the cell][parity][value]
    int flag[4];
};
__device__ __forceinline__ void mb_store(double* p, double v)
{
#ifdef IPC_MAILBOX_PLAIN
    *p = v;
#else
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
}
__device__ __forceinline__ double mb_load(const double* p)
{
#ifdef IPC_MAILBOX_PLAIN
    return *p;
#else
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
}

// what a wave does between two polls of its partner's mailbox flag
#ifndef IPC_SPIN_SLEEP
#define IPC_SPIN_SLEEP 1
#endif
#if IPC_SPIN_SLEEP > 0
#define IPC_SPIN_WAIT() __builtin_amdgcn_s_sleep(IPC_SPIN_SLEEP)
#else
#define IPC_SPIN_WAIT() asm volatile("s_nop 0")
#endif

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// SPD solve A x = b by LDL^T (N = 3 or 6) on wave-uniform values; reciprocals by v_rcp_f64 + two
// Newton steps.  Returns false when a pivot is not positive.
template <int N>
__device__ __forceinline__ bool ldl_solve(double (&A)[N][N], double (&b)[N])
{
    bool ok = true;
    double inv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k] * A[k][k];
        ok = ok && (d > 0);
        double r = __builtin_amdgcn_rcp(d);
        r = fma(fma(-d, r, 1.0), r, r);
        r = fma(fma(-d, r, 1.0), r, r);
        inv[j] = r;
        A[j][j] = d;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k] * A[k][k];
            A[i][j] = v * r;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= A[i][k] * b[k];
        b[i] = v;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) b[i] *= inv[i];
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double v = b[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) v -= A[k][i] * b[k];
        b[i] = v;
    }
    return ok;
}

// Gamma_l[i][a] of the capacitance assembly, from A = c_f cz - s_f sz, B = s_f cz + c_f sz (from-pose times measurement
// rotation), K = (-(y_t - y_g), x_t - x_g) and the loop's direction sigma.  Everything is formed first and then selected,
// so that i and a, which differ from lane to lane, cost selects and no branches.
__device__ __forceinline__ double se2_gamma(double Aq, double Bq, double Kx, double Ky, double sigma, int i, int a)
{
    const double g02 = Aq * Kx + Bq * Ky, g12 = -Bq * Kx + Aq * Ky, nB = -Bq;   // formed first: selects, not branches
    const double g0 = a == 0 ? Aq : (a == 1 ? Bq : g02);
    const double g1 = a == 0 ? nB : (a == 1 ? Aq : g12);
    const double g2 = a == 2 ? 1.0 : 0.0;
    const double g = i == 0 ? g0 : (i == 1 ? g1 : g2);
    return sigma * g;
}

template <int V> struct IntC { static constexpr int value = V; };

// The per-slot loops are fully unrolled (the state lives in registers).  Memory operations keep
// their source order, pure arithmetic does not: left alone it sinks towards its final uses, every
// operand loaded for the M slots stays live and the kernel spills (> 1000 VGPRs at M = 13).  An
// empty volatile asm that consumes the results of a slot pins that slot's arithmetic in place;
// the scheduling barrier keeps the next slot's loads behind it (measured: without it the kernels
// use a few registers less but C2 runs 6 % slower).
#define IPC_SLOT_FENCE() __builtin_amdgcn_sched_barrier(0)
#define IPC_PIN1(a) asm volatile("" : "+v"(a) : : "memory")
#define IPC_PIN2(a, b) asm volatile("" : "+v"(a), "+v"(b) : : "memory")
#define IPC_PIN3(a, b, c) asm volatile("" : "+v"(a), "+v"(b), "+v"(c) : : "memory")

// KEEP_E: the odometry errors of the committed state live in registers (3 doubles per pose), written by the commit
// sweep.  For large M they are recomputed from the poses where needed (~20 flops each) to stay inside the register
// file; a commit is then a pure pose update.
#ifndef IPC_KEEPE_MAX
#define IPC_KEEPE_MAX 8
#endif
// Look-ahead of the slot constants (PF below) up to this M; the one-wave kernels have room for it one step further.
#ifndef IPC_PF_MAX
#define IPC_PF_MAX 9
#endif
#ifndef IPC_PF_MAX_W1                                  // (a smaller IPC_PF_MAX, as -DIPC_PF_MAX=0, holds for them too)
#define IPC_PF_MAX_W1 (IPC_PF_MAX < 9 ? IPC_PF_MAX : 11)
#endif
// PARK_E (M = 9 and 11): phase A recomputes the errors as before and parks them in accumulator registers, by hand;
// phases B1 and C of the same iteration read them back instead of recomputing (the committed poses do not move in
// between), and no longer load the measurement translation and angle.  These kernels fill the vector registers: left
// to the register allocator, 6 M more live values come back as several hundred accumulator copies per dog-leg
// iteration, more than two recomputations cost.  Parked explicitly, a slot's three doubles cost six copies in phase A
// and six in each of B1 and C; nothing stays parked across the trial loop, and a commit remains a pure pose update
// (no neighbour exchange, no constants).  The parked value IS what err_of recomputes there: same bits.
// -DIPC_PARKE_SET=0 switches it off (bit i of the set: M = i).  M = 13 recomputes.
#ifndef IPC_PARKE_SET
#define IPC_PARKE_SET ((1 << 9) | (1 << 11))
#endif
// how se2_wave_solve holds the committed errors: 0 recomputed, 1 in vector registers (KEEP_E), 2 parked by phase A
template <int M>
constexpr int se2_err_store() { return M <= IPC_KEEPE_MAX ? 1 : (((IPC_PARKE_SET >> M) & 1) ? 2 : 0); }

struct ParkedE { int w[6]; };                        // three doubles as six accumulator registers
__device__ __forceinline__ void park_e(ParkedE& p, double e0, double e1, double e2)
{
    asm volatile("v_accvgpr_write_b32 %0, %6\n\tv_accvgpr_write_b32 %1, %7\n\tv_accvgpr_write_b32 %2, %8\n\t"
                 "v_accvgpr_write_b32 %3, %9\n\tv_accvgpr_write_b32 %4, %10\n\tv_accvgpr_write_b32 %5, %11"
                 : "=a"(p.w[0]), "=a"(p.w[1]), "=a"(p.w[2]), "=a"(p.w[3]), "=a"(p.w[4]), "=a"(p.w[5])
                 : "v"(__double2loint(e0)), "v"(__double2hiint(e0)), "v"(__double2loint(e1)), "v"(__double2hiint(e1)),
                   "v"(__double2loint(e2)), "v"(__double2hiint(e2)));
}
__device__ __forceinline__ void unpark_e(const ParkedE& p, double& e0, double& e1, double& e2)
{
    int l0, h0, l1, h1, l2, h2;
    asm volatile("v_accvgpr_read_b32 %0, %6\n\tv_accvgpr_read_b32 %1, %7\n\tv_accvgpr_read_b32 %2, %8\n\t"
                 "v_accvgpr_read_b32 %3, %9\n\tv_accvgpr_read_b32 %4, %10\n\tv_accvgpr_read_b32 %5, %11"
                 : "=v"(l0), "=v"(h0), "=v"(l1), "=v"(h1), "=v"(l2), "=v"(h2)
                 : "a"(p.w[0]), "a"(p.w[1]), "a"(p.w[2]), "a"(p.w[3]), "a"(p.w[4]), "a"(p.w[5]));
    e0 = __hiloint2double(h0, l0); e1 = __hiloint2double(h1, l1); e2 = __hiloint2double(h2, l2);
}

// KEEP_TRIAL: every trial sweep parks the pose it forms in each slot (x, y, theta, cos, sin: ten accumulator registers),
// and where the errors are kept (KEEP_E) the slot's three error values as a commit would store them.  An accepted trial
// is then committed by reading these back: no second sweep, so no stepping, no angle wrap, no rotation or sincos, and
// for KEEP_E no se2_error, no constants and no neighbour exchange (both waves of a pair skip it together, so their
// sequence numbers stay in step).  A rejected trial leaves X untouched and the next trial overwrites what was parked.
// The registers are those that pe (PARK_E) leaves dead during the trial loop plus the free accumulator registers; no
// vector register lives longer.  The parked values ARE what the commit sweep recomputes: same bits.
struct ParkedPose { int w[10]; };                    // x, y, theta, cos, sin as ten accumulator registers
__device__ __forceinline__ void park_pose(ParkedPose& p, const Pose2& Y)
{
    asm volatile("v_accvgpr_write_b32 %0, %10\n\tv_accvgpr_write_b32 %1, %11\n\tv_accvgpr_write_b32 %2, %12\n\t"
                 "v_accvgpr_write_b32 %3, %13\n\tv_accvgpr_write_b32 %4, %14\n\tv_accvgpr_write_b32 %5, %15\n\t"
                 "v_accvgpr_write_b32 %6, %16\n\tv_accvgpr_write_b32 %7, %17\n\tv_accvgpr_write_b32 %8, %18\n\t"
                 "v_accvgpr_write_b32 %9, %19"
                 : "=a"(p.w[0]), "=a"(p.w[1]), "=a"(p.w[2]), "=a"(p.w[3]), "=a"(p.w[4]), "=a"(p.w[5]), "=a"(p.w[6]),
                   "=a"(p.w[7]), "=a"(p.w[8]), "=a"(p.w[9])
                 : "v"(__double2loint(Y.x)), "v"(__double2hiint(Y.x)), "v"(__double2loint(Y.y)), "v"(__double2hiint(Y.y)),
                   "v"(__double2loint(Y.th)), "v"(__double2hiint(Y.th)), "v"(__double2loint(Y.c)), "v"(__double2hiint(Y.c)),
                   "v"(__double2loint(Y.s)), "v"(__double2hiint(Y.s)));
}
__device__ __forceinline__ void unpark_pose(const ParkedPose& p, Pose2& Y)
{
    int l0, h0, l1, h1, l2, h2, l3, h3, l4, h4;
    asm volatile("v_accvgpr_read_b32 %0, %10\n\tv_accvgpr_read_b32 %1, %11\n\tv_accvgpr_read_b32 %2, %12\n\t"
                 "v_accvgpr_read_b32 %3, %13\n\tv_accvgpr_read_b32 %4, %14\n\tv_accvgpr_read_b32 %5, %15\n\t"
                 "v_accvgpr_read_b32 %6, %16\n\tv_accvgpr_read_b32 %7, %17\n\tv_accvgpr_read_b32 %8, %18\n\t"
                 "v_accvgpr_read_b32 %9, %19"
                 : "=v"(l0), "=v"(h0), "=v"(l1), "=v"(h1), "=v"(l2), "=v"(h2), "=v"(l3), "=v"(h3), "=v"(l4), "=v"(h4)
                 : "a"(p.w[0]), "a"(p.w[1]), "a"(p.w[2]), "a"(p.w[3]), "a"(p.w[4]), "a"(p.w[5]), "a"(p.w[6]), "a"(p.w[7]),
                   "a"(p.w[8]), "a"(p.w[9]));
    Y.x = __hiloint2double(h0, l0); Y.y = __hiloint2double(h1, l1); Y.th = __hiloint2double(h2, l2);
    Y.c = __hiloint2double(h3, l3); Y.s = __hiloint2double(h4, l4);
}

// PARK_GAUGE (the lazy kernels at M = 9): the gauge pose -- the cell's pose 0, the same in every lane, written once per cell
// and read in every phase of every iteration -- lives in ten accumulator registers, by hand.  These kernels fill the vector
// registers to the last one; left to the register allocator, one of the gauge's doubles (x or y) goes to the accumulator
// file anyway and a second one no longer fits, which spills (lw9, lp9 un-staged: two spilled vector registers where kw9 and
// kp9 have none).  Parked explicitly, every use reads the doubles it needs back at that point -- x, y in phases B1, B2 and C,
// the whole pose where lane 0 takes it for its predecessor -- and no vector register holds any of it across the loop.
// Copies only: same bits.
struct ParkedD { int w[2]; };                        // one double as two accumulator registers
__device__ __forceinline__ void park_d(ParkedD& p, double v)
{
    asm volatile("v_accvgpr_write_b32 %0, %2\n\tv_accvgpr_write_b32 %1, %3"
                 : "=a"(p.w[0]), "=a"(p.w[1]) : "v"(__double2loint(v)), "v"(__double2hiint(v)));
}
__device__ __forceinline__ double unpark_d(const ParkedD& p)
{
    int l, h;
    asm volatile("v_accvgpr_read_b32 %0, %2\n\tv_accvgpr_read_b32 %1, %3" : "=v"(l), "=v"(h) : "a"(p.w[0]), "a"(p.w[1]));
    return __hiloint2double(h, l);
}

// LAZY_SD (the se2_*_kernel_lz kernels): b^T H b, alpha = b^T b / b^T H b and |h_sd| are read by a steepest-descent or
// dog-leg trial only, and most iterations accept the Gauss-Newton step at their first trial.  Phases B1 and B2 then form
// none of the three (no J b and quadratic form per slot, no information matrix loaded for it, no hand-off of b to the
// next lane -- in the pair kernels one mailbox exchange --, no b at the loop end points, no division, no square root);
// sd_terms() forms them, the same expressions reduced through the same network in the same order, at the first point of
// the trial loop that reads them: at most once per iteration, in most iterations never.  Same bits (see sd_terms).
//
// The reduction network of entry 1 of wave_sum16_store (block_prims.hpp) alone: that entry is b^T H b in phase B1.  Row 0
// of the packed value -- lanes l, l + 16, l + 32, l + 48 added as (l + (l + 32)) + ((l + 16) + (l + 48)), then the row
// scan -- takes nothing from the three entries packed beside it, so they are zeros here; lane 15 holds the sum.
__device__ __forceinline__ double wave_sum16_entry1(double v)
{
    const double r0 = pair32(v, 0.0);
    double q = pair16(r0, 0.0);
    q = row_inclusive_scan(q);
    return read_lane(q, 15);
}
// b^T b beyond this (or not a number) makes a LAZY_SD iteration form the steepest-descent terms at its head, as the other
// kernels do: see the trial loop.
constexpr double kLazySdMaxBb = 0x1p500;

template <int M, int NL, bool STAGED, int W = 1, int E_STORE = se2_err_store<M>(), bool KEEP_TRIAL = false,
          bool LAZY_SD = false>
__device__ __forceinline__ void se2_wave_solve(const Se2View& P, int lo_abs, int L, const int (&cand)[2], int iterations,
                               WaveScratch<NL>& sh, const double* cst, int wlo, int wstride, CellResult& res,
                               PairBox* box = nullptr, int seq0 = 0, int* seq_out = nullptr)
{
    static_assert(W == 1 || W == 2 || W == 4, "one, two or four cooperating waves per cell");
    constexpr bool KEEP_E = E_STORE == 1, PARK_E = E_STORE == 2;
    constexpr bool PARK_GAUGE = LAZY_SD && M == 9;
    // lp7 alone: "sd_terms ran in this iteration" is a bit of `flags`, not a wave-uniform bool of its own carried across the
    // trial loop (that one scalar state more cost lp7/nl1/staged two spilled scalar registers more than kp7 has); the bit
    // never leaves the function
    constexpr bool SD_BIT = LAZY_SD && M == 7 && W == 2;
    constexpr int kSdFormedBit = 0x100;
    constexpr int NS = NL * 3;
    const double term_scale = P.term_eps / (double)(L + NL);   // 0: the test is off
    bool lastGN = false;
    const int lane = threadIdx.x & 63;
    // wave of the cell: the same in every lane, and said so (readfirstlane), so that what depends on it alone -- which
    // mailbox rows to read, whose partial sum comes first -- is a scalar branch or select instead of an exec-mask skeleton
    const int wsub = W > 1 ? (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) & (W - 1)) : 0;
    const int gl = wsub * 64 + lane;                 // lane index within the cell
    int j0 = gl * M + 1;                             // pose index of slot 0 (not const: opaque() hides it)

    // ---- exchange among the W waves of the cell: every wave posts up to 8 doubles and waits for
    // all others; peer(o, k) then reads wave o's value k.  Also the cell's barrier. ----
#ifdef IPC_PHASE_TIMING
    unsigned long long gnEvals = 0, gnRejected = 0, nBig = 0, tmBig = 0, tmSmall = 0, nSd = 0;
    unsigned long long tmA = 0, tmB1 = 0, tmB2 = 0, tmC = 0, tmT = 0, tmW = 0, tmK = 0, tm0 = __builtin_amdgcn_s_memtime();
#define IPC_WTICK(acc) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); acc += t_ - tm0; tm0 = t_; }
#else
#define IPC_WTICK(acc)
#endif
    int seq = seq0;
    auto post_wait = [&](const double (&mine)[8], int n) {
        if constexpr (W > 1) {
            ++seq;
            double* my = box->data[wsub][seq & 1];
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 8; ++k) if (k < n) mb_store(&my[k], mine[k]);
            }
            wave_sync();
            if (lane == 0) __hip_atomic_store(&box->flag[wsub], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
#ifdef IPC_PHASE_TIMING
            const unsigned long long tw0 = __builtin_amdgcn_s_memtime();
#endif
#pragma unroll
            for (int o = 0; o < W; ++o) {
                if (o == wsub) continue;
                while (__hip_atomic_load(&box->flag[o], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - seq < 0)
                    IPC_SPIN_WAIT();
            }
#ifdef IPC_PHASE_TIMING
            tmW += __builtin_amdgcn_s_memtime() - tw0;
#endif
#ifdef IPC_MB_DELAY_WAVE                               // (protocol stress: one wave of the cell dawdles behind every exchange)
            if (wsub == IPC_MB_DELAY_WAVE) { __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); }
#endif
            // Every lane polls the flag with an acquire load above, so every lane's payload reads are ordered behind the
            // partner's release; the fence states that once more for the reads that follow, whatever the compiler makes of
            // the loop (LDS only: a fence over global memory would wait for the constant prefetches in flight).
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
            wave_sync();
        }
    };
    auto peer = [&](int o, int k) -> double { return mb_load(&box->data[o][seq & 1][k]); };
    auto pair_barrier = [&]() {
        if constexpr (W > 1) { double a[8] = {0, 0, 0, 0, 0, 0, 0, 0}; post_wait(a, 0); }
    };
    // sums over the cell of per-lane values: the waves' totals added in wave order on every wave
    auto cell_sum2 = [&](double v0, double v1, double& s0, double& s1) {
        const double t0 = wave_sum(v0), t1 = wave_sum(v1);
        if constexpr (W > 1) {
            double a[8] = {t0, t1, 0, 0, 0, 0, 0, 0};
            post_wait(a, 2);
#if defined(IPC_MAILBOX_PLAIN) && defined(IPC_DBG_SUM_SIDE)    // (tools/maxilp_repro.py: which wave's read goes wrong)
            auto rdx = [&](int o, int k) -> double {
                return ((IPC_DBG_SUM_SIDE >> o) & 1) ? __hip_atomic_load(&box->data[o][seq & 1][k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : peer(o, k);
            };
#else
            auto rdx = [&](int o, int k) -> double { return peer(o, k); };
#endif
            s0 = wsub == 0 ? t0 : rdx(0, 0);
            s1 = wsub == 0 ? t1 : rdx(0, 1);
#pragma unroll
            for (int o = 1; o < W; ++o) { s0 += o == wsub ? t0 : rdx(o, 0); s1 += o == wsub ? t1 : rdx(o, 1); }
        } else { s0 = t0; s1 = t1; }
    };
    // exclusive prefix over the cell's lanes of a per-lane total
    auto cell_excl = [&](double run) -> double {
        const double inc = wave_inclusive_scan(run);
        double off = inc - run;
        if constexpr (W > 1) {
            double a[8] = {read_lane(inc, 63), 0, 0, 0, 0, 0, 0, 0};
            post_wait(a, 1);
            double lower = 0.0;
#pragma unroll
            for (int o = 0; o < W - 1; ++o) if (o < wsub) lower += peer(o, 0);
            off += lower;
        }
        return off;
    };
    auto cell_excl2 = [&](double r0, double r1, double& o0, double& o1) {
        const double i0 = wave_inclusive_scan(r0), i1 = wave_inclusive_scan(r1);
        o0 = i0 - r0; o1 = i1 - r1;
        if constexpr (W > 1) {
            double a[8] = {read_lane(i0, 63), read_lane(i1, 63), 0, 0, 0, 0, 0, 0};
            post_wait(a, 2);
            double l0 = 0.0, l1 = 0.0;
#pragma unroll
            for (int o = 0; o < W - 1; ++o) if (o < wsub) { l0 += peer(o, 0); l1 += peer(o, 1); }
            o0 += l0; o1 += l1;
        }
    };

    // ---------------- loop constants -> LDS ----------------
    if (lane < NL && wsub == 0) {
        const int l = lane, c = cand[l];
        LoopConst& q = sh.lc[l];
        q.f = P.cand_from[c] - lo_abs;
        q.t = P.cand_to[c] - lo_abs;
        q.lo = min(q.f, q.t);
        q.hi = max(q.f, q.t);
        q.sigma = q.t > q.f ? 1.0 : -1.0;
        q.tzx = P.cand[(size_t)F_TZX * P.cstride + c];
        q.tzy = P.cand[(size_t)F_TZY * P.cstride + c];
        q.cz = P.cand[(size_t)F_CZ * P.cstride + c];
        q.sz = P.cand[(size_t)F_SZ * P.cstride + c];
        q.thz = P.cand[(size_t)F_THZ * P.cstride + c];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            q.om[k] = P.cand[(size_t)(F_OM + k) * P.cstride + c];
            q.sg[k] = P.cand[(size_t)(F_SG + k) * P.cstride + c];
        }
    }

    // ---------------- per-lane state ----------------
    Pose2 X[M];
    double ex[KEEP_E ? M : 1], ey[KEEP_E ? M : 1], eth[KEEP_E ? M : 1];
    ParkedE pe[PARK_E ? M : 1];                      // (phase A writes them before phases B1 and C read them)
    ParkedPose tY[KEEP_TRIAL ? M : 1];               // (a trial sweep writes them before an accepted trial reads them)
    ParkedE tE[(KEEP_TRIAL && KEEP_E) ? M : 1];
    double bx[M], by[M], bth[M];
    double hx[M], hy[M], hth[M];
    Pose2 gauge;
    gauge.x = P.pose0[lo_abs];
    gauge.y = P.pose0[(size_t)P.VS + lo_abs];
    gauge.th = P.pose0[(size_t)2 * P.VS + lo_abs];
    sincos_pi(gauge.th, gauge.s, gauge.c);
#pragma unroll
    for (int s = 0; s < M; ++s) {
        const int j = j0 + s;
        const int ja = j <= L ? lo_abs + j : lo_abs;
        X[s].x = P.pose0[ja];
        X[s].y = P.pose0[(size_t)P.VS + ja];
        X[s].th = P.pose0[(size_t)2 * P.VS + ja];
        sincos_pi(X[s].th, X[s].s, X[s].c);
        if (KEEP_E) ex[s] = ey[s] = eth[s] = 0.0;
        bx[s] = by[s] = bth[s] = 0.0;
        hx[s] = hy[s] = hth[s] = 0.0;
    }
    wave_sync();                                     // sh.lc visible
    pair_barrier();
    int lf[NL], lt[NL], of[NL], sf[NL], ot[NL], st_[NL], llo[NL], lhi[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        lf[l] = __builtin_amdgcn_readfirstlane(sh.lc[l].f);
        lt[l] = __builtin_amdgcn_readfirstlane(sh.lc[l].t);
        llo[l] = min(lf[l], lt[l]); lhi[l] = max(lf[l], lt[l]);
        of[l] = lf[l] > 0 ? (lf[l] - 1) / M : -1; sf[l] = lf[l] > 0 ? (lf[l] - 1) % M : -1;
        ot[l] = lt[l] > 0 ? (lt[l] - 1) / M : -1; st_[l] = lt[l] > 0 ? (lt[l] - 1) % M : -1;
    }
    // Slots of THIS wave that hold a loop end point (wave-uniform bit mask): the per-slot loops test
    // one bit instead of running the four owner checks in every slot.
    unsigned ownSlots = 0;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        if (of[l] >= 0 && (of[l] >> 6) == wsub) ownSlots |= 1u << sf[l];
        if (ot[l] >= 0 && (ot[l] >> 6) == wsub) ownSlots |= 1u << st_[l];
    }
    if (gl == 0) {                                   // gauge end points never change
#pragma unroll
        for (int l = 0; l < NL; ++l)
#pragma unroll
            for (int bsel = 0; bsel < 2; ++bsel) {
                double* pf = sh.ls[bsel][l].pf;
                double* pt = sh.ls[bsel][l].pt;
                if (lf[l] == 0) { pf[0] = gauge.x; pf[1] = gauge.y; pf[2] = gauge.th; pf[3] = gauge.c; pf[4] = gauge.s; }
                if (lt[l] == 0) { pt[0] = gauge.x; pt[1] = gauge.y; pt[2] = gauge.th; pt[3] = gauge.c; pt[4] = gauge.s; }
            }
        if constexpr (LAZY_SD) {                     // b at a gauge end point is zero, and sd_terms stores the other end points only
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                if (lf[l] == 0) { sh.lvec[l][0][0] = 0.0; sh.lvec[l][0][1] = 0.0; sh.lvec[l][0][2] = 0.0; }
                if (lt[l] == 0) { sh.lvec[l][1][0] = 0.0; sh.lvec[l][1][1] = 0.0; sh.lvec[l][1][2] = 0.0; }
            }
        }
    }

    // PARK_GAUGE: x, y, theta, cos, sin parked here, once per cell; `gauge` itself is not read below this point
    [[maybe_unused]] ParkedD pg[PARK_GAUGE ? 5 : 1];
    if constexpr (PARK_GAUGE) {
        park_d(pg[0], gauge.x); park_d(pg[1], gauge.y); park_d(pg[2], gauge.th); park_d(pg[3], gauge.c); park_d(pg[4], gauge.s);
    }
    auto gauge_x = [&]() -> double { if constexpr (PARK_GAUGE) return unpark_d(pg[0]); else return gauge.x; };
    auto gauge_y = [&]() -> double { if constexpr (PARK_GAUGE) return unpark_d(pg[1]); else return gauge.y; };
    auto gauge_pose = [&]() -> Pose2 {
        if constexpr (PARK_GAUGE) {
            Pose2 g;
            g.x = unpark_d(pg[0]); g.y = unpark_d(pg[1]); g.th = unpark_d(pg[2]); g.c = unpark_d(pg[3]); g.s = unpark_d(pg[4]);
            return g;
        } else return gauge;
    };

    // chain constants: local edge index of slot s is eloc + s (idle lanes are parked on edge 0;
    // the partially filled lane reads up to M-1 records past the chain, which the window padding
    // and the record-array padding cover)
    // The constants are loop-invariant, so the compiler would hoist every load out of the dog-leg
    // loop and pin 17 doubles per slot in registers; opaque() makes the index look modified, which
    // keeps the loads where they are used.  It hides two more per-lane values at every phase start:
    //   * j0: the predicates built on it (pose exists, pose inside loop l: ~5 M 64-bit lane masks) are
    //     then recomputed by a compare where they are used; hoisted out of the dog-leg loop they do not
    //     fit the scalar registers and come back as two v_readlane each;
    //   * the LDS address of the lane's first record, taken AFTER the window's base has been added: the
    //     base (the cells' scratch precedes the window) is beyond the 8-bit offsets of a paired LDS read,
    //     so with it left in the immediate every pair of loads paid a v_add_u32 of its own.
    int eloc = gl * M < L ? gl * M : 0;
    typedef const __attribute__((address_space(3))) double* LdsRec;
    LdsRec crec = nullptr;
    auto opaque = [&]() {
        asm volatile("" : "+v"(eloc), "+v"(j0));
        if (STAGED) { crec = (LdsRec)(cst + (lo_abs - wlo + eloc) * (int)F_SG); asm volatile("" : "+v"(crec)); }
    };
    auto ldc = [&](int field, int s) -> double {
        // staged window: one record of F_SG doubles per edge, so a slot's constants sit at
        // compile-time offsets from ONE per-lane address (no address arithmetic, paired reads);
        // with M odd the lane stride of M * 88 bytes is bank-conflict free
        if (STAGED && field < (int)F_SG) return crec[s * (int)F_SG + field];
        // HBM / L2: record-major copy of the chain, so these loads too are compile-time offsets
        // from one per-lane address
        return P.chain_rec[((size_t)(lo_abs + eloc) + s) * (int)F_NFIELDS + field];
    };
    auto ldsym = [&](int field0, int s) -> Sym3 {
        Sym3 m;
        m.a00 = ldc(field0 + 0, s); m.a01 = ldc(field0 + 1, s); m.a02 = ldc(field0 + 2, s);
        m.a11 = ldc(field0 + 3, s); m.a12 = ldc(field0 + 4, s); m.a22 = ldc(field0 + 5, s);
        return m;
    };
    // Constants of one slot, fetched ONE SLOT AHEAD of their use: the per-slot fences keep a slot's
    // loads inside that slot, so without the look-ahead every slot starts by waiting for its own LDS
    // (or L2) reads.  WANT bits: 1 measurement translation + angle, 2 measurement rotation,
    // 4 information, 8 covariance.
    struct SlotConst { double tzx, tzy, thz, cz, sz; Sym3 om, sg; };
    auto ld_slot = [&](int s, SlotConst& c, auto want_c) {
        constexpr int WANT = decltype(want_c)::value;
        if (WANT & 1) { c.tzx = ldc(F_TZX, s); c.tzy = ldc(F_TZY, s); c.thz = ldc(F_THZ, s); }
        if (WANT & 2) { c.cz = ldc(F_CZ, s); c.sz = ldc(F_SZ, s); }
        if (WANT & 4) c.om = ldsym(F_OM, s);
        if (WANT & 8) c.sg = ldsym(F_SG, s);
    };
    constexpr int kErrWant = KEEP_E ? 0 : 3;         // what err_of needs when the errors are recomputed
    constexpr int kErrWantBC = (KEEP_E || PARK_E) ? 0 : 3;   // ... in phases B1 and C, which read what phase A parked
    // the look-ahead costs one SlotConst of registers: only where the register file has room
    constexpr bool PF = M <= (W == 1 ? IPC_PF_MAX_W1 : IPC_PF_MAX);

    // pose j-1 of slot 0: slot M-1 of the lane below (lane 0 of the cell: the gauge; lane 0 of the
    // pair's second wave: lane 63 of the first, through the mailbox)
    auto prev0 = [&](const Pose2& last) -> Pose2 {
        Pose2 cr = gauge_pose();
        if constexpr (W > 1) {
            double a[8] = {read_lane(last.x, 63), read_lane(last.y, 63), read_lane(last.th, 63), read_lane(last.c, 63),
                           read_lane(last.s, 63), 0, 0, 0};
            post_wait(a, 5);
            if (wsub > 0) { cr.x = peer(wsub - 1, 0); cr.y = peer(wsub - 1, 1); cr.th = peer(wsub - 1, 2); cr.c = peer(wsub - 1, 3); cr.s = peer(wsub - 1, 4); }
        }
        Pose2 p;
        p.x = lane_prev(last.x, cr.x); p.y = lane_prev(last.y, cr.y); p.th = lane_prev(last.th, cr.th);
        p.c = lane_prev(last.c, cr.c); p.s = lane_prev(last.s, cr.s);
        return p;
    };
    // 3-vector of the lane below / above across the pair (0 at the ends of the cell)
    auto prev3 = [&](double vx, double vy, double vth, double& ox, double& oy, double& oth) {
        double c0 = 0.0, c1 = 0.0, c2 = 0.0;
        if constexpr (W > 1) {
            double a[8] = {read_lane(vx, 63), read_lane(vy, 63), read_lane(vth, 63), 0, 0, 0, 0, 0};
            post_wait(a, 3);
            if (wsub > 0) { c0 = peer(wsub - 1, 0); c1 = peer(wsub - 1, 1); c2 = peer(wsub - 1, 2); }
        }
        ox = lane_prev(vx, c0); oy = lane_prev(vy, c1); oth = lane_prev(vth, c2);
    };
    auto next3 = [&](double vx, double vy, double vth, double& ox, double& oy, double& oth) {
        double c0 = 0.0, c1 = 0.0, c2 = 0.0;
        if constexpr (W > 1) {
            double a[8] = {read_lane(vx, 0), read_lane(vy, 0), read_lane(vth, 0), 0, 0, 0, 0, 0};
            post_wait(a, 3);
            if (wsub < W - 1) { c0 = peer(wsub + 1, 0); c1 = peer(wsub + 1, 1); c2 = peer(wsub + 1, 2); }
        }
        ox = lane_next(vx, c0); oy = lane_next(vy, c1); oth = lane_next(vth, c2);
    };

    auto loop_eval = [&](int l, int bsel) -> double {
        const LoopConst& q = sh.lc[l];
        LoopState& st = sh.ls[bsel][l];
        Pose2 a{st.pf[0], st.pf[1], st.pf[2], st.pf[3], st.pf[4]};
        Pose2 b{st.pt[0], st.pt[1], st.pt[2], st.pt[3], st.pt[4]};
        double e0, e1, e2;
        se2_error(a, b, q.tzx, q.tzy, q.cz, q.sz, q.thz, e0, e1, e2);
        Sym3 om{q.om[0], q.om[1], q.om[2], q.om[3], q.om[4], q.om[5]};
        double q0, q1, q2;
        om.mul(e0, e1, e2, q0, q1, q2);
        const double chi = e0 * q0 + e1 * q1 + e2 * q2;
        st.e[0] = e0; st.e[1] = e1; st.e[2] = e2;
        st.chi = chi;
        return chi;
    };
    int cur = 0;
    auto loop_force = [&](int l) {
        const LoopConst& q = sh.lc[l];
        LoopState& st = sh.ls[cur][l];
        Sym3 om{q.om[0], q.om[1], q.om[2], q.om[3], q.om[4], q.om[5]};
        double q0, q1, q2;
        om.mul(st.e[0], st.e[1], st.e[2], q0, q1, q2);
        const double cP = st.pf[3] * q.cz - st.pf[4] * q.sz, sP = st.pf[4] * q.cz + st.pf[3] * q.sz;
        st.g[0] = cP * q0 - sP * q1; st.g[1] = sP * q0 + cP * q1; st.g[2] = q2;
    };

    // One sweep over the chain.
    //   MODE 0: errors of the committed poses X            -> e, chi2, loop state buffer `bsel`
    //   MODE 1: trial poses X (+) (p b + q h), not stored  -> chi2, loop state buffer `bsel`, changed
    //   MODE 2: commit X <- X (+) (p b + q h)              -> X, e
    // big (wave-uniform): some angle moves by >= 2^-6 rad (full sincos instead of the small
    // rotation).  A run-time flag on purpose: as two instantiations under one branch, the compiler
    // hoists the common half of every slot above the branch and keeps it alive.
    bool sweepChanged = false;
    // Identical sub-expressions recur in every phase (P_j, kappa_j, dt_j, range masks ...); the
    // compiler would keep them alive per slot from one phase to the next.  Laundering the state
    // at the phase boundaries (no instructions) makes it recompute them instead.
    auto launder = [&]() {
#pragma unroll
        for (int s = 0; s < M; ++s) {
            asm volatile("" : "+v"(X[s].x), "+v"(X[s].y), "+v"(X[s].c), "+v"(X[s].s));
            if (KEEP_E) asm volatile("" : "+v"(ex[s]), "+v"(ey[s]), "+v"(eth[s]));
        }
    };
    // error of edge j (slot s) at the committed poses: from registers, or recomputed
    auto err_of = [&](int s, const Pose2& a, const SlotConst& K, double& e0, double& e1, double& e2) {
        if (KEEP_E) { e0 = ex[s]; e1 = ey[s]; e2 = eth[s]; return; }
        se2_error(a, X[s], K.tzx, K.tzy, K.cz, K.sz, K.thz, e0, e1, e2);
        if (!(j0 + s <= L)) { e0 = 0.0; e1 = 0.0; e2 = 0.0; }
    };
    // the same in phases B1 and C: parked by phase A of this iteration (the committed poses have not moved since)
    auto err_again = [&](int s, const Pose2& a, const SlotConst& K, double& e0, double& e1, double& e2) {
        if (PARK_E) unpark_e(pe[s], e0, e1, e2);
        else err_of(s, a, K, e0, e1, e2);
    };
    // gn (wave-uniform): the step is exactly h (Gauss-Newton trial, p = 0, q = 1): X + (0 b + 1 h) and
    // X + h are the same bits, so the b operands and two operations per component are skipped.
    // wantChanged: only a steepest-descent trial needs to know whether any pose moved.
    auto sweep = [&](auto mode_c, bool big, double p, double q, int bsel, bool gn = false, bool wantChanged = true) -> double {
        constexpr int MODE = decltype(mode_c)::value;
        opaque();
        launder();
        // the commit sweep repeats the trial sweep's arithmetic; hide the coefficients so the
        // compiler cannot keep the trial's poses and errors alive to reuse them
        asm volatile("" : "+v"(p), "+v"(q));
        auto stepped = [&](int s) -> Pose2 {
            Pose2 Y;
            double dx, dy, dth;
            if (gn) { dx = hx[s]; dy = hy[s]; dth = hth[s]; }
            else { dx = fma(p, bx[s], q * hx[s]); dy = fma(p, by[s], q * hy[s]); dth = fma(p, bth[s], q * hth[s]); }
            Y.x = X[s].x + dx;
            Y.y = X[s].y + dy;
            Y.th = wrap_pi(X[s].th + dth);
            if (big) sincos_pi(Y.th, Y.s, Y.c);
            else rotate_small(X[s].c, X[s].s, Y.th - X[s].th, Y.c, Y.s);
            return Y;
        };
        const Pose2 last = MODE == 0 ? X[M - 1] : stepped(M - 1);
        Pose2 prev = last;
        if (MODE != 2 || KEEP_E) prev = prev0(last);  // (a commit without stored errors needs no neighbour)
        double part = 0.0;
        bool changed = false;
        constexpr int kWant = (MODE != 2 || KEEP_E) ? (MODE != 2 ? 7 : 3) : 0;
        SlotConst Kn;
        if (PF) ld_slot(0, Kn, IntC<kWant>{});
#pragma unroll
        for (int s = 0; s < M; ++s) {
            SlotConst K;
            if (PF) { K = Kn; if (s + 1 < M) ld_slot(s + 1, Kn, IntC<kWant>{}); }
            else ld_slot(s, K, IntC<kWant>{});
            const Pose2 Y = MODE == 0 ? X[s] : (s == M - 1 ? last : stepped(s));
            const bool v = j0 + s <= L;
            if (MODE == 1 && wantChanged) changed |= v && ((Y.x != X[s].x) || (Y.y != X[s].y) || (Y.th != X[s].th));
            double e0 = 0.0, e1 = 0.0, e2 = 0.0;
            if (MODE != 2 || KEEP_E) se2_error(prev, Y, K.tzx, K.tzy, K.cz, K.sz, K.thz, e0, e1, e2);
            if (MODE != 2) {
                const double c2 = K.om.quad(e0, e1, e2);
                part += v ? c2 : 0.0;
            }
            if (MODE != 1 && KEEP_E) { ex[s] = v ? e0 : 0.0; ey[s] = v ? e1 : 0.0; eth[s] = v ? e2 : 0.0; }
            if constexpr (MODE == 1 && KEEP_TRIAL) {
                park_pose(tY[s], Y);
                if constexpr (KEEP_E) park_e(tE[s], v ? e0 : 0.0, v ? e1 : 0.0, v ? e2 : 0.0);
            }
            if (MODE != 2 && ((ownSlots >> s) & 1u)) {
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    if (sf[l] == s && gl == of[l]) {
                        double* w = sh.ls[bsel][l].pf;
                        w[0] = Y.x; w[1] = Y.y; w[2] = Y.th; w[3] = Y.c; w[4] = Y.s;
                    }
                    if (st_[l] == s && gl == ot[l]) {
                        double* w = sh.ls[bsel][l].pt;
                        w[0] = Y.x; w[1] = Y.y; w[2] = Y.th; w[3] = Y.c; w[4] = Y.s;
                    }
                }
            }
            if (MODE == 2) X[s] = Y;
            prev = Y;
            if (MODE != 2) IPC_PIN1(part);
            if (MODE != 1 && KEEP_E) IPC_PIN3(ex[s], ey[s], eth[s]);
            if (MODE == 2) IPC_PIN3(X[s].x, X[s].y, X[s].th);
            IPC_PIN3(prev.x, prev.y, prev.th);
            IPC_PIN2(prev.c, prev.s);
            IPC_SLOT_FENCE();
        }
        if (MODE == 2) return 0.0;
        wave_sync();
        if constexpr (W > 1) {
            // one exchange: the partial sums of both waves; it also tells each wave that the
            // partner's loop end points are in place, so the loops are evaluated after it (by both
            // waves, same values; the first wave's lanes store the loop state)
            double tot, chg;
            cell_sum2(part, (MODE == 1 && changed) ? 1.0 : 0.0, tot, chg);
            const double lc = lane < NL ? loop_eval(lane, bsel) : 0.0;
#pragma unroll
            for (int l = 0; l < NL; ++l) tot += read_lane(lc, l);
            if (MODE == 1) sweepChanged = chg != 0.0;
            return tot;
        } else {
            if (lane < NL) part += loop_eval(lane, bsel);
            double tot, chg;
            cell_sum2(part, (MODE == 1 && changed) ? 1.0 : 0.0, tot, chg);
            if (MODE == 1) sweepChanged = chg != 0.0;
            return tot;
        }
    };

    // ---------------- initial errors (consensus_utils.cpp:11) ----------------
    int evals = 1;
    double currentChi = sweep(IntC<0>{}, false, 0.0, 0.0, cur);

    // ---------------- dog-leg (g2o OptimizationAlgorithmDogleg::solve) ----------------
    double delta = 1e4;
    const int maxTrials = 100;
    int it_done = 0, tries_total = 0, flags = 0;

    IPC_WTICK(tmT)
    for (int it = 0; it < iterations; ++it) {
        // ---- phase A: forces g, hand-back m -> b ----
        opaque();
        launder();
        if (gl < NL) loop_force(gl);
        wave_sync();
        const Pose2 a0 = prev0(X[M - 1]);             // (also orders the loop forces before their readers)
        constexpr int kWantA = 2 | 4 | kErrWant;
        auto force = [&](int s, const Pose2& a, const SlotConst& K, double& gx, double& gy, double& gth, double& mx,
                         double& my, double& mth) {
            const double cz = K.cz, sz = K.sz;
            const double cP = a.c * cz - a.s * sz, sP = a.s * cz + a.c * sz;
            double e0, e1, e2, qx, qy, qth;
            err_of(s, a, K, e0, e1, e2);                                // zero on idle slots
            if (PARK_E) park_e(pe[s], e0, e1, e2);
            K.om.mul(e0, e1, e2, qx, qy, qth);
            gx = cP * qx - sP * qy;
            gy = sP * qx + cP * qy;
            gth = qth;
            const double dx = X[s].x - a.x, dy = X[s].y - a.y;
            mx = gx; my = gy;
            mth = gth + (-dy * gx + dx * gy);
        };
        double bbp = 0.0;
        {
            double g0x, g0y, g0th, m0x, m0y, m0th;
            SlotConst Kn;
            {
                SlotConst K0;
                ld_slot(0, K0, IntC<kWantA>{});
                if (PF && M > 1) ld_slot(M - 1, Kn, IntC<kWantA>{});
                force(0, a0, K0, g0x, g0y, g0th, m0x, m0y, m0th);
            }
            double nx, ny, nth;
            next3(m0x, m0y, m0th, nx, ny, nth);
#pragma unroll
            for (int s = M - 1; s >= 0; --s) {
                double gx, gy, gth, mx, my, mth;
                if (s == 0) { gx = g0x; gy = g0y; gth = g0th; mx = m0x; my = m0y; mth = m0th; }
                else {
                    SlotConst K;
                    if (PF) { K = Kn; if (s - 1 > 0) ld_slot(s - 1, Kn, IntC<kWantA>{}); }
                    else ld_slot(s, K, IntC<kWantA>{});
                    force(s, X[s - 1], K, gx, gy, gth, mx, my, mth);
                }
                const bool v = j0 + s <= L;
                double tx = nx - gx, ty = ny - gy, tth = nth - gth;
                if ((ownSlots >> s) & 1u) {
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    const LoopState& st = sh.ls[cur][l];
                    if (st_[l] == s && gl == ot[l]) { tx -= st.g[0]; ty -= st.g[1]; tth -= st.g[2]; }
                    if (sf[l] == s && gl == of[l]) {
                        const double dx = st.pt[0] - st.pf[0], dy = st.pt[1] - st.pf[1];
                        tx += st.g[0]; ty += st.g[1];
                        tth += st.g[2] + (-dy * st.g[0] + dx * st.g[1]);
                    }
                }
                }
                bx[s] = v ? tx : 0.0; by[s] = v ? ty : 0.0; bth[s] = v ? tth : 0.0;
                bbp += bx[s] * bx[s] + by[s] * by[s] + bth[s] * bth[s];
                nx = mx; ny = my; nth = mth;
                IPC_PIN3(bx[s], by[s], bth[s]);
                IPC_PIN3(nx, ny, nth);
                IPC_PIN1(bbp);
                IPC_SLOT_FENCE();
            }
        }
        IPC_WTICK(tmA)
        // ---- phase B: b^T b, b^T H b, capacitance partials, solve ----
        double bb, bHb, alpha, hsdNorm;
        double nu[NL][3];
        opaque();
        launder();
        {
            // b at the loop end points (the gauge end point carries zero)
            if constexpr (!LAZY_SD) {
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                if (gl == 0) {
                    if (lf[l] == 0) { sh.lvec[l][0][0] = 0.0; sh.lvec[l][0][1] = 0.0; sh.lvec[l][0][2] = 0.0; }
                    if (lt[l] == 0) { sh.lvec[l][1][0] = 0.0; sh.lvec[l][1][1] = 0.0; sh.lvec[l][1][2] = 0.0; }
                }
#pragma unroll
                for (int s = 0; s < M; ++s) {
                    if (!((ownSlots >> s) & 1u)) continue;
                    if (sf[l] == s && gl == of[l]) { sh.lvec[l][0][0] = bx[s]; sh.lvec[l][0][1] = by[s]; sh.lvec[l][0][2] = bth[s]; }
                    if (st_[l] == s && gl == ot[l]) { sh.lvec[l][1][0] = bx[s]; sh.lvec[l][1][1] = by[s]; sh.lvec[l][1][2] = bth[s]; }
                }
            }
            }
            // group 1: b^T b, b^T H b, W_1 (3), M_11 (6); group 2: W_2 (3), M_22 (6), M_12 (6)
            // (LAZY_SD: entry 1 stays zero here, sd_terms reduces b^T H b where a trial reads it)
            double v1[16], v2[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) { v1[k] = 0.0; v2[k] = 0.0; }
            v1[0] = bbp;
            double qbx, qby, qbth;
            if constexpr (!LAZY_SD) prev3(bx[M - 1], by[M - 1], bth[M - 1], qbx, qby, qbth);
            constexpr int kWantB = 2 | (LAZY_SD ? 0 : 4) | 8 | kErrWantBC;
            SlotConst Kn;
            if (PF) ld_slot(0, Kn, IntC<kWantB>{});
#pragma unroll
            for (int s = 0; s < M; ++s) {
                SlotConst K;
                if (PF) { K = Kn; if (s + 1 < M) ld_slot(s + 1, Kn, IntC<kWantB>{}); }
                else ld_slot(s, K, IntC<kWantB>{});
                const Pose2& a = s == 0 ? a0 : X[s - 1];
                const bool v = j0 + s <= L;
                const double cz = K.cz, sz = K.sz;
                if constexpr (!LAZY_SD) {
                double wx, wy, wth;
                se2_apply_J(a, X[s], cz, sz, qbx, qby, qbth, bx[s], by[s], bth[s], wx, wy, wth);
                const double hq = K.om.quad(wx, wy, wth);
                v1[1] += v ? hq : 0.0;
                }
                const Sym3 sg = K.sg;
                const double c = a.c * cz - a.s * sz, sn = a.s * cz + a.c * sz;
                const double kx = -(X[s].y - gauge_y()), ky = X[s].x - gauge_x();
                const double cc = c * c, ss = sn * sn, cs = c * sn;
                const double C00 = cc * sg.a00 - 2 * cs * sg.a01 + ss * sg.a11;
                const double C01 = cs * (sg.a00 - sg.a11) + (cc - ss) * sg.a01;
                const double C11 = ss * sg.a00 + 2 * cs * sg.a01 + cc * sg.a11;
                const double c0 = c * sg.a02 - sn * sg.a12, c1 = sn * sg.a02 + c * sg.a12;
                const double sth = sg.a22;
                double psi[6];
                psi[2] = c0 - sth * kx;
                psi[4] = c1 - sth * ky;
                psi[0] = C00 - kx * c0 - kx * psi[2];
                psi[1] = C01 - kx * c1 - ky * psi[2];
                psi[3] = C11 - ky * c1 - ky * psi[4];
                psi[5] = sth;
                double e0, e1, e2;
                err_again(s, a, K, e0, e1, e2);
                const double w0 = c * e0 - sn * e1 - kx * e2;
                const double w1 = sn * e0 + c * e1 - ky * e2;
                const double w2 = e2;
                const int j = j0 + s;
                const double m1 = (v && j > llo[0] && j <= lhi[0]) ? 1.0 : 0.0;
                v1[2] += m1 * w0; v1[3] += m1 * w1; v1[4] += m1 * w2;
#pragma unroll
                for (int k = 0; k < 6; ++k) v1[5 + k] += m1 * psi[k];
                if constexpr (NL == 2) {
                    const double m2 = (v && j > llo[1] && j <= lhi[1]) ? 1.0 : 0.0;
                    const double m12 = m1 * m2;
                    v2[0] += m2 * w0; v2[1] += m2 * w1; v2[2] += m2 * w2;
#pragma unroll
                    for (int k = 0; k < 6; ++k) { v2[3 + k] += m2 * psi[k]; v2[9 + k] += m12 * psi[k]; }
                }
                if constexpr (!LAZY_SD) { qbx = bx[s]; qby = by[s]; qbth = bth[s]; }
                if constexpr (LAZY_SD)
                    asm volatile("" : "+v"(v1[0]), "+v"(v1[2]), "+v"(v1[3]), "+v"(v1[4]), "+v"(v1[5]),
                                 "+v"(v1[6]), "+v"(v1[7]), "+v"(v1[8]), "+v"(v1[9]), "+v"(v1[10]) : : "memory");
                else
                asm volatile("" : "+v"(v1[0]), "+v"(v1[1]), "+v"(v1[2]), "+v"(v1[3]), "+v"(v1[4]), "+v"(v1[5]),
                             "+v"(v1[6]), "+v"(v1[7]), "+v"(v1[8]), "+v"(v1[9]), "+v"(v1[10]) : : "memory");
                if constexpr (NL == 2)
                    asm volatile("" : "+v"(v2[0]), "+v"(v2[1]), "+v"(v2[2]), "+v"(v2[3]), "+v"(v2[4]), "+v"(v2[5]),
                                 "+v"(v2[6]), "+v"(v2[7]), "+v"(v2[8]), "+v"(v2[9]), "+v"(v2[10]), "+v"(v2[11]),
                                 "+v"(v2[12]), "+v"(v2[13]), "+v"(v2[14]) : : "memory");
                IPC_SLOT_FENCE();
            }
            wave_sum16_store(v1, &sh.red[wsub][0]);
            if constexpr (NL == 2) wave_sum16_store(v2, &sh.red[wsub][16]);
            wave_sync();
            pair_barrier();                           // both waves' partial sums and end-point vectors are in place
            IPC_WTICK(tmB1)
            // ---- capacitance solve, lane-parallel (a uniform 6x6 solve in registers would pin ~150
            // VGPRs while the whole chain state is live):
            //   lane r*(NS+1)+c  : S[r][c] (c < NS) / rhs d[r] (c == NS), then Gauss-Jordan in place
            // With one wave per SIMD nothing hides an LDS round trip, so the block makes as few as it can:
            //   * every LDS operand (loop constants and state, the partial sums, the end-point vectors) is fetched
            //     once, as one batch, with indices clamped instead of predicated so that no branch splits the batch;
            //   * lane l*9+i*3+a forms Gamma_l[i][a] (se2_gamma) and the lanes of S fetch the six entries they use
            //     with cross-lane reads issued together: one round trip instead of a store to LDS, a wave_sync and
            //     serialised re-reads;
            //   * what does not depend on the solve sits under those reads (the sums over the cell's waves, the loops'
            //     part of b^T H b) and under the pivots' cross-lane reads and reciprocals (alpha, |h_sd|);
            //   * nu's cross-lane reads (three of mu, three of Gamma's column) are issued together.
            constexpr int RS = NS + 1;                    // row stride of the augmented system
            // The lane's place in the system is recomputed here in every iteration: derived from `lane` itself, the
            // indices and the dozen lane masks are hoisted out of the dog-leg loop and live (spilled) across all of it.
            int bl = lane;
            asm volatile("" : "+v"(bl));
            const int r = bl / RS, c = bl % RS;
            const bool inS = bl < NS * RS;
            const int l1 = (NL > 1 && inS) ? r / 3 : 0, i = r % 3;     // loop / component of the row
            const int l2 = (NL > 1 && c < NS) ? c / 3 : 0, k3 = c % 3; // ... of the column (k3 also: nu's column)
            const int lq_l = bl < NL ? bl : 0;
            // -- the batch --
            // Gamma: lane l*9+i*3+a forms Gamma_l[i][a] (the lanes beyond form loop 0's again; nobody reads them)
            const int g_l = (NL > 1 && bl < NL * 9) ? bl / 9 : 0, g_i = (bl % 9) / 3, g_a = bl % 3;
            const LoopConst& qg = sh.lc[g_l];
            const LoopState& sg_ = sh.ls[cur][g_l];
            const double gcz = qg.cz, gsz = qg.sz, gsig = qg.sigma;
            const double gpc = sg_.pf[3], gps = sg_.pf[4], gtx = sg_.pt[0], gty = sg_.pt[1];
            const double s1e = sh.ls[cur][l1].e[i];
            // partial sums of the row's block, M_{l1 l2} (6 values), and of the row's right-hand side, W_{l1} (3).  (The
            // rhs lanes could take W through M's per-lane base and share its sums: 6 FP64 instructions less, but the
            // static FP64 count of the loop body is how tests/test_se2_loop_mix.py sees that the arithmetic is untouched.)
            const int mb = l1 == l2 ? (l1 == 0 ? 5 : 19) : 25, wb = l1 == 0 ? 2 : 16;
            double mred[W][6], wred[W][3], bred[W][2];
#pragma unroll
            for (int o = 0; o < W; ++o) {
#pragma unroll
                for (int k = 0; k < 6; ++k) mred[o][k] = sh.red[o][mb + k];
#pragma unroll
                for (int k = 0; k < 3; ++k) wred[o][k] = sh.red[o][wb + k];
                bred[o][0] = sh.red[o][0];
                if constexpr (!LAZY_SD) bred[o][1] = sh.red[o][1];
            }
            const int lo_ = i < k3 ? i : k3, hi_ = i < k3 ? k3 : i;
            const double sgv = sh.lc[l1].sg[lo_ * 3 - lo_ * (lo_ - 1) / 2 + (hi_ - lo_)];
            // operands of the loops' own b^T H b term (lanes >= NL read loop 0's and drop the result; LAZY_SD: sd_terms)
            Pose2 qa, qb;
            double qcz, qsz;
            Sym3 qom;
            double qv[2][3];
            if constexpr (!LAZY_SD) {
            const LoopConst& qq = sh.lc[lq_l];
            const LoopState& sq = sh.ls[cur][lq_l];
            qa = Pose2{sq.pf[0], sq.pf[1], sq.pf[2], sq.pf[3], sq.pf[4]};
            qb = Pose2{sq.pt[0], sq.pt[1], sq.pt[2], sq.pt[3], sq.pt[4]};
            qcz = qq.cz; qsz = qq.sz;
            qom = Sym3{qq.om[0], qq.om[1], qq.om[2], qq.om[3], qq.om[4], qq.om[5]};
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int k = 0; k < 3; ++k) qv[e][k] = sh.lvec[lq_l][e][k];
            }
            __builtin_amdgcn_sched_barrier(0);
            // -- Gamma, and its entries to the lanes that use them: row i of loop l1 and row k3 of loop l2 for S[r][c],
            // six cross-lane reads, one wait (nu's column of Gamma is fetched with mu, behind the pivots) --
            double g1[3], g2[3], gam;
            {
                const double Aq = gpc * gcz - gps * gsz, Bq = gps * gcz + gpc * gsz;
                const double Kx = -(gty - gauge_y()), Ky = gtx - gauge_x();
                gam = se2_gamma(Aq, Bq, Kx, Ky, gsig, g_i, g_a);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    g1[a] = __shfl(gam, l1 * 9 + i * 3 + a, 64);
                    g2[a] = __shfl(gam, l2 * 9 + k3 * 3 + a, 64);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            // under them, independent of Gamma: the sums over the cell's waves and the loops' b^T H b term
            double m[6], w[3];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                m[k] = mred[0][k];
#pragma unroll
                for (int o = 1; o < W; ++o) m[k] += mred[o][k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                w[k] = wred[0][k];
#pragma unroll
                for (int o = 1; o < W; ++o) w[k] += wred[o][k];
            }
            bb = bred[0][0];
            if constexpr (LAZY_SD) {
                bHb = 0.0;
#pragma unroll
                for (int o = 1; o < W; ++o) bb += bred[o][0];
                IPC_PIN1(bb);
            } else {
            bHb = bred[0][1];
#pragma unroll
            for (int o = 1; o < W; ++o) { bb += bred[o][0]; bHb += bred[o][1]; }
            {
                double wx, wy, wth;                        // (loop_quad)
                se2_apply_J(qa, qb, qcz, qsz, qv[0][0], qv[0][1], qv[0][2], qv[1][0], qv[1][1], qv[1][2], wx, wy, wth);
                const double lq = bl < NL ? qom.quad(wx, wy, wth) : 0.0;
#pragma unroll
                for (int l = 0; l < NL; ++l) bHb += read_lane(lq, l);
            }
            IPC_PIN2(bb, bHb);
            }
            __builtin_amdgcn_sched_barrier(0);
            // -- assembly --
            double val;
            {
                const double g10 = g1[0], g11 = g1[1], g12 = g1[2];
                const double m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[3], m12 = m[4], m22 = m[5];
                const double t0 = g10 * m00 + g11 * m01 + g12 * m02;
                const double t1 = g10 * m01 + g11 * m11 + g12 * m12;
                const double t2 = g10 * m02 + g11 * m12 + g12 * m22;
                double vS = t0 * g2[0] + t1 * g2[1] + t2 * g2[2];
                const double vSd = vS + sgv;
                vS = l1 == l2 ? vSd : vS;
                const double vR = s1e - (g10 * w[0] + g11 * w[1] + g12 * w[2]);
                val = c < NS ? vS : vR;
                val = inS ? val : 0.0;
            }
            bool okS = true;
            alpha = 0.0; hsdNorm = 0.0;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const double rowk = __shfl(val, k * RS + c, 64);
                const double colk = __shfl(val, r * RS + k, 64);
                __builtin_amdgcn_sched_barrier(0);         // the two cross-lane reads go first; the rest runs under them
                const double piv = read_lane(val, k * RS + k);
                okS = okS && (piv > 0);
                double inv = __builtin_amdgcn_rcp(piv);
                inv = fma(fma(-piv, inv, 1.0), inv, inv);
                inv = fma(fma(-piv, inv, 1.0), inv, inv);
                // independent of the solve
                if constexpr (!LAZY_SD) {
                if (k == 0) {
                    alpha = bb / bHb;
                    IPC_PIN1(alpha);
                } else if (k == 1) {
                    hsdNorm = sqrt(alpha * alpha * bb);
                    IPC_PIN1(hsdNorm);
                }
                }
                __builtin_amdgcn_sched_barrier(0);
                val = (r == k) ? rowk * inv : fma(-(colk * rowk), inv, val);
            }
            {   // nu_l[cc] = sum_rr Gamma_l[rr][cc] mu_{3l+rr}; mu_r sits in lane r*RS + NS.  Formed in the lanes
                // (row 3l, column cc).
                double mu[3], gn[3];
#pragma unroll
                for (int rr = 0; rr < 3; ++rr) {
                    mu[rr] = __shfl(val, (3 * l1 + rr) * RS + NS, 64);
                    gn[rr] = __shfl(gam, l1 * 9 + rr * 3 + k3, 64);
                }
                double nv = 0.0;
#pragma unroll
                for (int rr = 0; rr < 3; ++rr) nv += gn[rr] * mu[rr];
#pragma unroll
                for (int l = 0; l < NL; ++l)
#pragma unroll
                    for (int k = 0; k < 3; ++k) nu[l][k] = read_lane(nv, 3 * l * RS + k);
            }
            if (!okS) { flags |= 2; break; }
        }
        IPC_WTICK(tmB2)
        // ---- phase C: u, rho, prefix sums -> h_gn; |h|^2, b.h (h^T H h = b.h) ----
        double hgnNorm, bh, hHh;
        opaque();
        launder();
        {
            // rho into (hx, hy, hth); theta prefix in-lane
            double run = 0.0;
            constexpr int kWantC = 2 | 8 | kErrWantBC;
            SlotConst Kn;
            if (PF) ld_slot(0, Kn, IntC<kWantC>{});
#pragma unroll
            for (int s = 0; s < M; ++s) {
                SlotConst K;
                if (PF) { K = Kn; if (s + 1 < M) ld_slot(s + 1, Kn, IntC<kWantC>{}); }
                else ld_slot(s, K, IntC<kWantC>{});
                const Pose2& a = s == 0 ? a0 : X[s - 1];
                const int j = j0 + s;
                const bool v = j <= L;
                const double m1 = (v && j > llo[0] && j <= lhi[0]) ? 1.0 : 0.0;
                double n0 = m1 * nu[0][0], n1 = m1 * nu[0][1], n2 = m1 * nu[0][2];
                if constexpr (NL == 2) {
                    const double m2 = (v && j > llo[1] && j <= lhi[1]) ? 1.0 : 0.0;
                    n0 += m2 * nu[1][0]; n1 += m2 * nu[1][1]; n2 += m2 * nu[1][2];
                }
                const double cz = K.cz, sz = K.sz;
                const double c = a.c * cz - a.s * sz, sn = a.s * cz + a.c * sz;
                const double kx = -(X[s].y - gauge_y()), ky = X[s].x - gauge_x();
                const double wx = c * n0 + sn * n1, wy = -sn * n0 + c * n1, wth = -(kx * n0 + ky * n1) + n2;
                double vx, vy, vth;
                K.sg.mul(wx, wy, wth, vx, vy, vth);
                double e0, e1, e2;
                err_again(s, a, K, e0, e1, e2);
                const double ux = -vx - e0, uy = -vy - e1, uth = -vth - e2;
                hx[s] = v ? c * ux - sn * uy : 0.0;
                hy[s] = v ? sn * ux + c * uy : 0.0;
                run += v ? uth : 0.0;
                hth[s] = run;                        // in-lane inclusive prefix of rho_theta
                IPC_PIN3(hx[s], hy[s], hth[s]);
                IPC_SLOT_FENCE();
            }
            const double offT = cell_excl(run);                        // h_theta of the lane's predecessor pose
            double rx = 0.0, ry = 0.0, thPrev = offT;
#pragma unroll
            for (int s = 0; s < M; ++s) {
                const Pose2& a = s == 0 ? a0 : X[s - 1];
                const bool v = j0 + s <= L;
                hth[s] += offT;
                const double dx = X[s].x - a.x, dy = X[s].y - a.y;
                rx += v ? hx[s] - dy * thPrev : 0.0;
                ry += v ? hy[s] + dx * thPrev : 0.0;
                hx[s] = rx; hy[s] = ry;
                thPrev = hth[s];
                IPC_PIN3(hx[s], hy[s], hth[s]);
                IPC_SLOT_FENCE();
            }
            double offX, offY;
            cell_excl2(rx, ry, offX, offY);
            double p0 = 0.0, p1 = 0.0;
#pragma unroll
            for (int s = 0; s < M; ++s) {
                const bool v = j0 + s <= L;
                hx[s] = v ? hx[s] + offX : 0.0;
                hy[s] = v ? hy[s] + offY : 0.0;
                hth[s] = v ? hth[s] : 0.0;
                p0 += hx[s] * hx[s] + hy[s] * hy[s] + hth[s] * hth[s];
                p1 += bx[s] * hx[s] + by[s] * hy[s] + bth[s] * hth[s];
            }
            double hh;
            cell_sum2(p0, p1, hh, bh);
            hgnNorm = sqrt(hh);
            hHh = bh;
        }
        IPC_WTICK(tmC)
        // converged (Se2View::term_eps): in the Newton regime (the last iteration took the full Gauss-Newton
        // step at its first trial) and one more such step cannot move any edge's chi2 by more than
        // 2 sqrt(term_eps) relative; g2o would still run its trial loop to Terminate
        if (lastGN && hgnNorm < delta && fabs(bh) < term_scale * currentChi) { it_done = it + 1; tries_total += maxTrials; flags |= 1; break; }
        // ---- steepest-descent terms of a LAZY_SD kernel: b^T H b, alpha, |h_sd|, what phases B1 and B2 left out ----
        // The same bits as there: the per-slot term is the same two helpers on the same operands (the committed poses and
        // b have not moved: no trial has been accepted yet); a lane adds its slots from 0.0 in slot order with the same
        // select; the wave's sum goes through entry 1's place in wave_sum16_store's network; the waves' sums are added in
        // wave order and the loops' own terms after them in loop order; alpha and |h_sd| are the same expressions.
        // Pairs: both waves enter together -- the caller branches on the cell sums, delta and the trial count, which both
        // waves hold bit-identically -- and run the same two exchanges, so their sequence numbers stay in step.  The first
        // exchange carries what prev0 and prev3 carry apart elsewhere (the first wave's last pose and last b: 8 values).
        // sh.lvec is written and read nowhere else in these kernels and sh.red not at all here (the wave's sum crosses
        // in the mailbox).  A wave's lvec stores precede its post of the first exchange and both waves read lvec behind
        // the second; the next sd_terms (a later iteration) stores again only behind the exchanges of at least one trial
        // sweep, which a wave passes only after its partner has posted them, that is after the partner's reads above in
        // its program order (LDS operations of one wave complete in order).  The partner's B2 reads of sh.red and of the
        // loop state lie before its phase C exchanges, which this wave has passed.
        [[maybe_unused]] bool sdReady = false;
        if constexpr (SD_BIT) flags &= ~kSdFormedBit;
        [[maybe_unused]] auto sd_terms = [&]() {
#ifdef IPC_PHASE_TIMING
            ++nSd;
#endif
            // (two comments in the assembly, each behind a scheduling barrier: tools/isa_loop_mix.py counts the block apart)
            __builtin_amdgcn_sched_barrier(0);
            asm volatile(";ipc_sd_terms_begin" : : : "memory");
            opaque();
            launder();
            // b at the loop end points (the gauge end point carries zero: stored once, with the gauge's pose, before the loop)
#pragma unroll
            for (int l = 0; l < NL; ++l) {
#pragma unroll
                for (int s = 0; s < M; ++s) {
                    if (!((ownSlots >> s) & 1u)) continue;
                    if (sf[l] == s && gl == of[l]) { sh.lvec[l][0][0] = bx[s]; sh.lvec[l][0][1] = by[s]; sh.lvec[l][0][2] = bth[s]; }
                    if (st_[l] == s && gl == ot[l]) { sh.lvec[l][1][0] = bx[s]; sh.lvec[l][1][1] = by[s]; sh.lvec[l][1][2] = bth[s]; }
                }
            }
            // pose j-1 and b of the lane below
            Pose2 cr = gauge_pose();
            double c0 = 0.0, c1 = 0.0, c2 = 0.0;
            if constexpr (W > 1) {
                double a[8] = {read_lane(X[M - 1].x, 63), read_lane(X[M - 1].y, 63), read_lane(X[M - 1].th, 63),
                               read_lane(X[M - 1].c, 63), read_lane(X[M - 1].s, 63),
                               read_lane(bx[M - 1], 63), read_lane(by[M - 1], 63), read_lane(bth[M - 1], 63)};
                post_wait(a, 8);
                if (wsub > 0) {
                    cr.x = peer(wsub - 1, 0); cr.y = peer(wsub - 1, 1); cr.th = peer(wsub - 1, 2); cr.c = peer(wsub - 1, 3);
                    cr.s = peer(wsub - 1, 4);
                    c0 = peer(wsub - 1, 5); c1 = peer(wsub - 1, 6); c2 = peer(wsub - 1, 7);
                }
            } else {
                wave_sync();                          // sh.lvec visible
            }
            Pose2 as0;
            as0.x = lane_prev(X[M - 1].x, cr.x); as0.y = lane_prev(X[M - 1].y, cr.y); as0.th = lane_prev(X[M - 1].th, cr.th);
            as0.c = lane_prev(X[M - 1].c, cr.c); as0.s = lane_prev(X[M - 1].s, cr.s);
            double qbx = lane_prev(bx[M - 1], c0), qby = lane_prev(by[M - 1], c1), qbth = lane_prev(bth[M - 1], c2);
            double acc = 0.0;
            constexpr int kWantS = 2 | 4;
            SlotConst Kn;
            if (PF) ld_slot(0, Kn, IntC<kWantS>{});
#pragma unroll
            for (int s = 0; s < M; ++s) {
                SlotConst K;
                if (PF) { K = Kn; if (s + 1 < M) ld_slot(s + 1, Kn, IntC<kWantS>{}); }
                else ld_slot(s, K, IntC<kWantS>{});
                const Pose2& a = s == 0 ? as0 : X[s - 1];
                const bool v = j0 + s <= L;
                const double cz = K.cz, sz = K.sz;
                double wx, wy, wth;
                se2_apply_J(a, X[s], cz, sz, qbx, qby, qbth, bx[s], by[s], bth[s], wx, wy, wth);
                const double hq = K.om.quad(wx, wy, wth);
                acc += v ? hq : 0.0;
                qbx = bx[s]; qby = by[s]; qbth = bth[s];
                IPC_PIN1(acc);
                IPC_SLOT_FENCE();
            }
            const double t = wave_sum16_entry1(acc);
            if constexpr (W > 1) {
                double a[8] = {t, 0, 0, 0, 0, 0, 0, 0};
                post_wait(a, 1);
                bHb = wsub == 0 ? t : peer(0, 0);
#pragma unroll
                for (int o = 1; o < W; ++o) bHb += o == wsub ? t : peer(o, 0);
            } else {
                bHb = t;
            }
            {
                // the loops' own term (lanes >= NL read loop 0's operands and drop the result)
                int bl = lane;
                asm volatile("" : "+v"(bl));
                const int lq_l = bl < NL ? bl : 0;
                const LoopConst& qq = sh.lc[lq_l];
                const LoopState& sq = sh.ls[cur][lq_l];
                const Pose2 qa{sq.pf[0], sq.pf[1], sq.pf[2], sq.pf[3], sq.pf[4]};
                const Pose2 qb{sq.pt[0], sq.pt[1], sq.pt[2], sq.pt[3], sq.pt[4]};
                const double qcz = qq.cz, qsz = qq.sz;
                const Sym3 qom{qq.om[0], qq.om[1], qq.om[2], qq.om[3], qq.om[4], qq.om[5]};
                double qv[2][3];
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int k = 0; k < 3; ++k) qv[e][k] = sh.lvec[lq_l][e][k];
                double wx, wy, wth;                        // (loop_quad)
                se2_apply_J(qa, qb, qcz, qsz, qv[0][0], qv[0][1], qv[0][2], qv[1][0], qv[1][1], qv[1][2], wx, wy, wth);
                const double lq = bl < NL ? qom.quad(wx, wy, wth) : 0.0;
#pragma unroll
                for (int l = 0; l < NL; ++l) bHb += read_lane(lq, l);
            }
            alpha = bb / bHb;
            hsdNorm = sqrt(alpha * alpha * bb);
            IPC_PIN3(bHb, alpha, hsdNorm);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile(";ipc_sd_terms_end" : : : "memory");
        };
        // ---- trial loop ----
        const double deltaAtEntry = delta;
        bool goodStep = false, dlReady = false;
        double dlC = 0.0, dlBma = 0.0;
        int numTries = 0;
        do {
            ++numTries;
            if constexpr (LAZY_SD) {
                // The first point of this iteration that reads b^T H b, alpha or |h_sd|: a trial that is not Gauss-Newton,
                // the first one or the one after a rejected Gauss-Newton trial (whose retry loop has taken delta down to
                // |h_gn| or below; once a trial is not Gauss-Newton none of this iteration is again).  A Gauss-Newton trial
                // reads b^T H b in one place, h_dl^T H h_dl = p p bHb + 2 p q bb + q q hHh with p = 0.0 and q = 1.0, and
                // evaluates it with bHb = 0.0 here.  The bits are those of the finite b^T H b: p p bHb is then +0 or -0;
                // 2 p q bb is +0 exactly, since bb, a sum of squares, is not negative; (+-0) + (+0) is +0 under round to
                // nearest, also where the two are contracted into one fused multiply-add (the exact product +-0 plus +0);
                // so what is added to q q hHh is +0 in both kernels, whatever the sign of b^T H b.  b h_dl = p bb + q bh
                // does not hold b^T H b.  Only a b^T H b that is infinite or not a number differs: 0 times it poisons the
                // gain and the other kernels then stop the cell.  So where bb is not a number or beyond 2^500 the terms
                // are formed before the first trial whatever its type, as the other kernels do.  Below the bound every
                // component of b is below 2^250 in magnitude, a slot's J b is at most (2 + 2 |r|) times two of them (r the
                // edge's relative translation, the rotations are unit), and its quadratic form at most nine times the
                // largest information entry times that squared, and a sum of finite terms of this size stays finite.  That
                // is finite UNDER AN ASSUMPTION ON THE DATA, which nothing here enforces: information entries and distances
                // between neighbouring poses below 2^160.  Data beyond it would give the other kernels a gain that is not a
                // number where this one's is finite.
                // (every lane holds the same values; the ballot says so, which makes this a scalar branch)
                if constexpr (SD_BIT) {
                    if (!(flags & kSdFormedBit) && __ballot(!(hgnNorm < delta) || !(bb <= kLazySdMaxBb)) != 0ull) { sd_terms(); flags |= kSdFormedBit; }
                } else
                if (!sdReady && __ballot(!(hgnNorm < delta) || !(bb <= kLazySdMaxBb)) != 0ull) { sd_terms(); sdReady = true; }
            }
            int stepType;                             // 0 GN, 1 SD, 2 DL
            double beta = 0.0, sdScale = 0.0;
            if (hgnNorm < delta) stepType = 0;
            else if (hsdNorm > delta) { stepType = 1; sdScale = delta / hsdNorm; }
            else {
                stepType = 2;
                // c = hsd.(hgn-hsd) and |hgn-hsd|^2 do not depend on delta: reduced once per iteration, reused by
                // every later dog-leg trial of the same iteration (same bits)
                if (!dlReady) {
                    double p0 = 0.0, p1 = 0.0;
#pragma unroll
                    for (int s = 0; s < M; ++s) {
                        const double sx = alpha * bx[s], sy = alpha * by[s], sth = alpha * bth[s];
                        const double ax = hx[s] - sx, ay = hy[s] - sy, ath = hth[s] - sth;
                        p0 += sx * ax + sy * ay + sth * ath;
                        p1 += ax * ax + ay * ay + ath * ath;
                    }
                    cell_sum2(p0, p1, dlC, dlBma);
                    dlReady = true;
                }
                const double c = dlC, bma = dlBma;
                const double hsdSq = alpha * alpha * bb;
                if (c <= 0.) beta = (-c + sqrt(c * c + bma * (delta * delta - hsdSq))) / bma;
                else beta = (delta * delta - hsdSq) / (c + sqrt(c * c + bma * (delta * delta - hsdSq)));
            }
            double pcoef, qcoef, hdlNorm;
            if (stepType == 0) { pcoef = 0.0; qcoef = 1.0; hdlNorm = hgnNorm; }
            else if (stepType == 1) { pcoef = sdScale * alpha; qcoef = 0.0; hdlNorm = delta; }
            else { pcoef = alpha - beta * alpha; qcoef = beta; hdlNorm = delta; }
            const double hdlHhdl = pcoef * pcoef * bHb + 2 * pcoef * qcoef * bb + qcoef * qcoef * hHh;
            const double bhdl = pcoef * bb + qcoef * bh;
            double linearGain = -1 * hdlHhdl + 2 * bhdl;
            bool big = false;
            double pc2 = pcoef, qc2 = qcoef;
            asm volatile("" : "+v"(pc2), "+v"(qc2));
#pragma unroll
            for (int s = 0; s < M; ++s) {
                const double thn = wrap_pi(X[s].th + (stepType == 0 ? hth[s] : fma(pc2, bth[s], qc2 * hth[s])));
                big |= fabs(thn - X[s].th) >= 0.015625;
            }
            const bool anyBig = __ballot(big) != 0ull;
            const int trial = cur ^ 1;
#ifdef IPC_PHASE_TIMING
            const unsigned long long tb0 = __builtin_amdgcn_s_memtime();
#endif
            const double newChi = sweep(IntC<1>{}, anyBig, pcoef, qcoef, trial, stepType == 0, stepType == 1);
#ifdef IPC_PHASE_TIMING
            if (anyBig) { ++nBig; tmBig += __builtin_amdgcn_s_memtime() - tb0; } else { tmSmall += __builtin_amdgcn_s_memtime() - tb0; }
#endif
            const bool anyChanged = stepType == 1 ? sweepChanged : true;
            ++evals;
            const double nonLinearGain = currentChi - newChi;
#ifdef IPC_PHASE_TIMING
            if (stepType == 0) { ++gnEvals; if (!(linearGain > 0 ? nonLinearGain > 0 : nonLinearGain < 0)) ++gnRejected; }
#endif
            if (fabs(linearGain) < 1e-12) linearGain = 1e-12;
            const bool linPos = linearGain > 0;
            auto rho_gt = [&](double t) { return linPos ? nonLinearGain > t * linearGain : nonLinearGain < t * linearGain; };
            auto rho_lt = [&](double t) { return linPos ? nonLinearGain < t * linearGain : nonLinearGain > t * linearGain; };
            if (rho_gt(0.0)) {                        // rho > 0, discardTop: commit the trial
                goodStep = true;
                currentChi = newChi;
                cur = trial;
                IPC_WTICK(tmT)
                if constexpr (KEEP_TRIAL) {
#pragma unroll
                    for (int s = 0; s < M; ++s) {
                        unpark_pose(tY[s], X[s]);
                        // Pinned as the commit sweep pins what it writes, in the pair kernels only: there it keeps a value that
                        // lives across the whole solve (gauge.x) in its vector register in kp9, in the one-wave kernels the
                        // same pin moves two more such values of kw9 to accumulator registers.
                        if constexpr (W > 1) IPC_PIN3(X[s].x, X[s].y, X[s].th);
                        if constexpr (KEEP_E) unpark_e(tE[s], ex[s], ey[s], eth[s]);
                    }
                } else {
                    sweep(IntC<2>{}, anyBig, pcoef, qcoef, trial, stepType == 0, false);
                }
                IPC_WTICK(tmK)
            }
            if (rho_gt(0.75)) delta = fmax(delta, 3 * hdlNorm);
            else if (rho_lt(0.25)) delta *= 0.5;
            if (!goodStep) {
                if (nonLinearGain != nonLinearGain) {
                    numTries = maxTrials;       // NaN gain ratio: g2o leaves delta alone, so every retry is this same trial
                } else if (stepType == 0) {
                    while (numTries < maxTrials && hgnNorm < delta) { ++numTries; delta *= 0.5; }
                } else if (stepType == 1 && !anyChanged) {
                    numTries = maxTrials;
                }
            }
        } while (!goodStep && numTries < maxTrials);
        lastGN = goodStep && numTries == 1 && hgnNorm < deltaAtEntry;
        it_done = it + 1;
        tries_total += numTries;
        IPC_WTICK(tmT)
        if (numTries == maxTrials || !goodStep) { flags |= 1; break; }
    }
#ifdef IPC_PHASE_TIMING
    if (lane == 0 && wsub == 0 && P.dbg) {
        unsigned long long* d = reinterpret_cast<unsigned long long*>(P.dbg) + 64 + 16 * (M + 16 * (W - 1));
        atomicAdd(d + 0, tmA); atomicAdd(d + 1, tmB1); atomicAdd(d + 2, tmB2); atomicAdd(d + 3, tmC);
        atomicAdd(d + 4, tmT); atomicAdd(d + 5, tmW);
        atomicAdd(d + 6, (unsigned long long)it_done); atomicAdd(d + 7, (unsigned long long)evals);
        atomicAdd(d + 8, (unsigned long long)it_done * (unsigned long long)L);
        atomicAdd(d + 9, 1ull); atomicAdd(d + 10, tmK); atomicAdd(d + 11, (unsigned long long)(evals - 1 - it_done)); atomicAdd(d + 12, gnEvals); atomicAdd(d + 13, gnRejected); atomicAdd(d + 14, nBig); atomicAdd(d + 15, tmBig); atomicAdd(d + 1024, tmSmall);
        if constexpr (LAZY_SD) atomicAdd(d + 1025, nSd);      // iterations that ran sd_terms
    }
#endif

    // ---- per-edge chi2 (consensus_utils.cpp:15-19) ----
    double mx = 0.0;
    bool nan = false;
    opaque();
    {
        const Pose2 a0 = prev0(X[M - 1]);
#pragma unroll
        for (int s = 0; s < M; ++s) {
            SlotConst K;
            ld_slot(s, K, IntC<(4 | kErrWant)>{});
            double e0, e1, e2;
            err_of(s, s == 0 ? a0 : X[s - 1], K, e0, e1, e2);
            if (j0 + s > L) continue;
            const double c = K.om.quad(e0, e1, e2);
            if (c != c) nan = true;
            else mx = fmax(mx, c);
        }
    }
    mx = wave_max(mx);
    nan = __ballot(nan) != 0ull;
    if constexpr (W > 1) {
        double a[8] = {mx, nan ? 1.0 : 0.0, 0, 0, 0, 0, 0, 0};
        post_wait(a, 2);
#pragma unroll
        for (int o = 0; o < W; ++o) {
            if (o == wsub) continue;
            mx = fmax(mx, peer(o, 0));
            nan = nan || peer(o, 1) != 0.0;
        }
    }
    wave_sync();
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const double c = sh.ls[cur][l].chi;
        if (c != c) nan = true;
        else mx = fmax(mx, c);
    }
    // consensus_utils.cpp:17-19 rejects as soon as ONE edge has chi2 > th; a NaN chi2 is not "> th".  So the maximum is
    // taken over the edges that have a number, and NaN is reported only when none of them is positive (agrees either way).
    if (nan && !(mx > 0.0)) mx = __longlong_as_double(0x7ff8000000000000ll);
    res.max_chi2 = mx;
    res.chi2_total = currentChi;
    res.iterations = it_done;
    res.tries = tries_total;
    res.flags = SD_BIT ? flags & ~kSdFormedBit : flags;
    res.evals = evals;
    if (seq_out) *seq_out = seq;
}

}  // namespace ipc
