// The cell plan: which kernel serves the cells of which chain length.  Host code only -- the table of the cell kernels
// (one descriptor per instantiation, expanded from the lists of cell_kernels.hpp), the policy strings, make_plan and the
// choice of the kernel of one launch.  Needs the view and parameter types as names only, so a plain host program can
// include it with stub launchers (tests/host/cell_plan_main.cpp).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cell_kernels.hpp"

// ------------------------------------------------------------------------------------------
// kernel variants: (threads per cell, poses per thread); capacity = T*M poses
// ------------------------------------------------------------------------------------------
// (global scope: BinCaps is an argument of the planning kernels, so its name is part of their symbols)
constexpr int kMaxBins = 32;
struct BinCaps { int n; int cap[kMaxBins]; };

namespace ipc {

enum class CellFamily { block, wave, pair, quad, lds, wave_kt, pair_kt, wave_lz, pair_lz };

// One compiled cell kernel.  se2 / se3: the launcher of its family, for the pose type of its table (the other is null).
struct CellKernel {
    const char* token;                                 // its policy token; a lazy kernel's tag ("lwM" / "lpM") is no token
    CellFamily family;
    int W, M;
    IPC_CELL_LAUNCHER((*se2), Se2View);
    IPC_CELL_LAUNCHER((*se3), Se3View);
    int capacity() const { return 64 * W * M; }
};

// Equal capacities are served in the order of these tables (make_plan): block kernels in the order of their list, then
// w, p, q (SE3: the LDS-pose kernels), kw, kp.
#define IPC_K2(tok, fam, WW, MM) {tok, CellFamily::fam, WW, MM, launch_se2_##fam, nullptr},
#define IPC_K3(tok, fam, WW, MM) {tok, CellFamily::fam, WW, MM, nullptr, launch_se3_##fam},
#define IPC_K_BLOCK2(WW, MM) IPC_K2(#WW "x" #MM, block, WW, MM)
#define IPC_K_WAVE(MM) IPC_K2("w" #MM, wave, 1, MM)
#define IPC_K_PAIR(MM) IPC_K2("p" #MM, pair, 2, MM)
#define IPC_K_QUAD(MM) IPC_K2("q" #MM, quad, 4, MM)
#define IPC_K_WAVE_KT(MM) IPC_K2("kw" #MM, wave_kt, 1, MM)
#define IPC_K_PAIR_KT(MM) IPC_K2("kp" #MM, pair_kt, 2, MM)
#define IPC_K_WAVE_LZ(MM) IPC_K2("lw" #MM, wave_lz, 1, MM)
#define IPC_K_PAIR_LZ(MM) IPC_K2("lp" #MM, pair_lz, 2, MM)
#define IPC_K_BLOCK3(WW, MM) IPC_K3(#WW "x" #MM, block, WW, MM)
#define IPC_K_LDS(WW, MM) IPC_K3((WW == 1 ? "w" #MM : "g" #MM), lds, WW, MM)
static const CellKernel kSe2Kernels[] = {
    IPC_SE2_BLOCK_WM(IPC_K_BLOCK2) IPC_SE2_WAVE_M(IPC_K_WAVE) IPC_SE2_PAIR_M(IPC_K_PAIR) IPC_SE2_QUAD_M(IPC_K_QUAD)
    IPC_SE2_WAVE_KT_M(IPC_K_WAVE_KT) IPC_SE2_PAIR_KT_M(IPC_K_PAIR_KT) IPC_SE2_WAVE_LZ_M(IPC_K_WAVE_LZ) IPC_SE2_PAIR_LZ_M(IPC_K_PAIR_LZ)
};
static const CellKernel kSe3Kernels[] = { IPC_SE3_BLOCK_WM(IPC_K_BLOCK3) IPC_SE3_LDS_WM(IPC_K_LDS) };
#undef IPC_K_LDS
#undef IPC_K_BLOCK3
#undef IPC_K_PAIR_LZ
#undef IPC_K_WAVE_LZ
#undef IPC_K_PAIR_KT
#undef IPC_K_WAVE_KT
#undef IPC_K_QUAD
#undef IPC_K_PAIR
#undef IPC_K_WAVE
#undef IPC_K_BLOCK2
#undef IPC_K3
#undef IPC_K2

static const CellKernel* find_kernel(int dim, CellFamily family, int W, int M)
{
    const CellKernel* k = dim == 2 ? kSe2Kernels : kSe3Kernels;
    const CellKernel* end = dim == 2 ? std::end(kSe2Kernels) : std::end(kSe3Kernels);
    for (; k != end; ++k) if (k->family == family && k->W == W && k->M == M) return k;
    return nullptr;
}

// Chain-length bins: each bin is served by one (W, M) kernel variant.  The policy string
// (env IPC_SE2_POLICY, default below) lists the variants to use as "WxM" tokens (block kernel, W
// waves per cell, M poses per lane), "wM" tokens (SE2 wave kernel, one wave per cell, M poses per
// lane), "pM" tokens (SE2 pair kernel, two waves per cell), "qM" tokens (SE2 quad kernel, four
// waves per cell) or "kwM" / "kpM" tokens (the kept-trial form of the wave / pair kernel, same capacity and
// results: DESIGN.md 4.1); a cell goes to the listed variant of
// smallest capacity 64*W*M that holds it.
struct BinPlan {
    BinCaps caps;
    const CellKernel* kernel[kMaxBins];
    // SE3: variant for a bin with too few cells to fill the GPU (more waves per cell, so the few
    // cells finish sooner), and the cell count below which it is used
    const CellKernel* latency[kMaxBins];
    int latency_below[kMaxBins];
    // SE2: the lazy steepest-descent form that serves the bin's kernel (same cells, same bits; lazy_sd_serves below)
    const CellKernel* lazy[kMaxBins];
};
// kwM / kpM where the kept-trial kernel passed its static and its measured gate: not at M = 11, whose
// kept-trial kernels spill to scratch and run slower than w11 / p11
static const char* kDefaultPolicy = "w1,w3,kw5,kw7,kw9,w11,w13,kp7,kp9,p11,q7,q9,q11,q13,16x4,16x8,16x16";
// The lazy steepest-descent kernels (se2_wave_lz.hip / se2_pair_lz.hip, LAZY_SD of se2_wave_solve) are not variants of
// their own: each computes, bit for bit, what one kernel of the default policy computes, so it has no token, no capacity
// and no place in a policy string -- a bin whose variant is that kernel is served by the lazy one.  IPC_SE2_LAZY_SD=0
// (read with the policy) switches the substitution off: every token then launches the kernel it names, which is the A/B
// partner inside one library; =2 substitutes every M that has a lazy kernel, listed below or not (the bitwise test and
// the per-bin gate runs reach the unlisted ones that way).  Only the M listed here are substituted by default: the
// kernels that passed the static gate (tests/test_se2_lazy_sd_loop_mix.py) and the measured one
// (profiles/se2_lazy_sd_c2_kernel_gate.txt, profiles/se2_lazy_gauge_c2_kernel_gate.txt).
// Every one of the eight is faster in its bin on the MI355X; lw9 and lp9 are listed since they park the gauge pose in
// accumulator registers by hand (PARK_GAUGE, se2_wave_cell.hpp: no spilled vector register in any instantiation) and lp7
// since its "terms formed" flag is a bit of the flags word (SD_BIT: no more spilled scalar registers than kp7); lw13 is
// held back by its scratch: DESIGN.md 8 has the figures.
static const int kLazySdWaveM[] = {5, 7, 9, 11};         // for kw5, kw7, kw9, w11 (not 13: w13)
static const int kLazySdPairM[] = {7, 9, 11};            // for kp7, kp9, p11
// The lazy kernel that serves k, or null.  every: any kernel that has a lazy form (IPC_SE2_LAZY_SD=2, tests and gate runs)
static const CellKernel* lazy_sd_serves(const CellKernel& k, bool every)
{
    const bool kept = k.family == CellFamily::wave_kt || k.family == CellFamily::pair_kt;
    const bool wave = k.family == CellFamily::wave || k.family == CellFamily::wave_kt;
    const bool pair = k.family == CellFamily::pair || k.family == CellFamily::pair_kt;
    // a lazy kernel is the kept-trial kernel up to M = kLazyKeepTrialMaxM and the re-sweeping one beyond
    if ((!wave && !pair) || kept != (k.M <= kLazyKeepTrialMaxM)) return nullptr;
    const CellKernel* lz = find_kernel(2, wave ? CellFamily::wave_lz : CellFamily::pair_lz, k.W, k.M);
    if (!lz || every) return lz;
    if (wave) for (int m : kLazySdWaveM) if (m == k.M) return lz;
    if (pair) for (int m : kLazySdPairM) if (m == k.M) return lz;
    return nullptr;
}
static const char* kDefaultPolicy3 = "w1,w2,w3,w4,w6,w8,g3,g4,g5,g6,g7,g8,g9,g10,16x4";
static const char* kBlockPolicy3 = "1x1,1x2,1x3,2x2,2x3,4x2,4x4,8x4,8x5,16x4";   // round-1 block kernels only (IPC_SE3_POLICY=block)
// SE3 variants for thin bins, by capacity (IPC_SE3_LATENCY_POLICY; "none" disables the switch)
static const char* kDefaultLatencyPolicy3 = "1x1,2x1,4x1,4x2,4x4,8x4,8x5,16x4";

// One policy string -> its kernels in the order of service: by capacity, equal capacities in table order.  On an error,
// tok is the token at fault.  block_only: any other family's token is a bad one (the latency policy).
enum class PolicyError { none, bad_token, not_compiled };
static PolicyError parse_policy(const std::string& pol, int dim, bool block_only, std::vector<const CellKernel*>& out, std::string& tok)
{
    for (size_t pos = 0, e; pos < pol.size(); pos = e + 1) {
        e = pol.find(',', pos);
        if (e == std::string::npos) e = pol.size();
        tok = pol.substr(pos, e - pos);
        const char* s = tok.c_str();
        CellFamily f = CellFamily::block;
        int w = 0, m = 0;
        if (dim == 2 && sscanf(s, "kw%d", &m) == 1) { f = CellFamily::wave_kt; w = 1; }       // (before "w%d": a prefix, not a suffix, names it)
        else if (dim == 2 && sscanf(s, "kp%d", &m) == 1) { f = CellFamily::pair_kt; w = 2; }
        else if (dim == 2 && sscanf(s, "w%d", &m) == 1) { f = CellFamily::wave; w = 1; }
        else if (dim == 2 && sscanf(s, "p%d", &m) == 1) { f = CellFamily::pair; w = 2; }
        else if (dim == 2 && sscanf(s, "q%d", &m) == 1) { f = CellFamily::quad; w = 4; }
        else if (dim == 3 && (sscanf(s, "w%d", &m) == 1 || sscanf(s, "g%d", &m) == 1)) { f = CellFamily::lds; w = s[0] == 'w' ? 1 : 4; }
        else if (sscanf(s, "%dx%d", &w, &m) != 2) return PolicyError::bad_token;
        if (block_only && f != CellFamily::block) return PolicyError::bad_token;
        const CellKernel* k = find_kernel(dim, f, w, m);
        if (!k) return PolicyError::not_compiled;
        out.push_back(k);
    }
    std::sort(out.begin(), out.end(), [](const CellKernel* a, const CellKernel* b) {
        return a->capacity() != b->capacity() ? a->capacity() < b->capacity() : a < b;
    });
    return PolicyError::none;
}

static bool make_plan(BinPlan& bp, int dim, std::string& err)
{
    const char* env = getenv(dim == 2 ? "IPC_SE2_POLICY" : "IPC_SE3_POLICY");
    std::string pol = env && *env ? env : (dim == 2 ? kDefaultPolicy : kDefaultPolicy3);
    if (dim == 3 && pol == "block") pol = kBlockPolicy3;
    std::vector<const CellKernel*> items;
    std::string tok;
    switch (parse_policy(pol, dim, false, items, tok)) {
        case PolicyError::bad_token: err = "bad IPC_SE2_POLICY token"; return false;
        case PolicyError::not_compiled: err = "IPC_SE*_POLICY names a variant that is not compiled: " + tok; return false;
        case PolicyError::none: break;
    }
    if (items.empty() || (int)items.size() > kMaxBins) { err = "IPC_SE2_POLICY: 1..32 variants"; return false; }
    bp.caps.n = (int)items.size();
    for (int b = 0; b < kMaxBins; ++b) {
        bp.caps.cap[b] = b < bp.caps.n ? items[b]->capacity() : 0;
        bp.kernel[b] = b < bp.caps.n ? items[b] : nullptr;
        bp.latency[b] = nullptr;
        bp.latency_below[b] = 0;
        bp.lazy[b] = nullptr;
    }
    if (dim == 2) {
        const char* lz = getenv("IPC_SE2_LAZY_SD");
        if (lz && *lz && strcmp(lz, "0") != 0 && strcmp(lz, "1") != 0 && strcmp(lz, "2") != 0) { err = "IPC_SE2_LAZY_SD: 0, 1 or 2"; return false; }
        const bool lazy_on = !(lz && *lz == '0'), every = lz && *lz == '2';
        for (int b = 0; b < bp.caps.n; ++b) bp.lazy[b] = lazy_on ? lazy_sd_serves(*bp.kernel[b], every) : nullptr;
    }
    if (dim == 3) {
        const char* lenv = getenv("IPC_SE3_LATENCY_POLICY");
        const std::string lpol = lenv && *lenv ? lenv : kDefaultLatencyPolicy3;
        if (lpol != "none") {
            std::vector<const CellKernel*> lat;
            switch (parse_policy(lpol, dim, true, lat, tok)) {
                case PolicyError::bad_token: err = "bad IPC_SE3_LATENCY_POLICY token"; return false;
                case PolicyError::not_compiled: err = "IPC_SE3_LATENCY_POLICY names a variant that is not compiled"; return false;
                case PolicyError::none: break;
            }
            for (int b = 0; b < bp.caps.n; ++b) {
                if (bp.kernel[b]->family != CellFamily::block) continue;     // block variants only
                const int wt = bp.kernel[b]->W;
                for (const CellKernel* lv : lat) {
                    if (lv->capacity() < bp.caps.cap[b]) continue;
                    // only a variant with more waves per cell is a latency variant
                    if (lv->W > wt) {
                        bp.latency[b] = lv;
                        bp.latency_below[b] = wt <= 4 ? 4 / wt : 1;      // x CUs at launch time
                    }
                    break;
                }
            }
        }
    }
    return true;
}

// The kernel that solves the n cells of bin b in one launch: the latency variant of a thin bin, else the lazy form
// that serves the bin's kernel, else the bin's own.
inline const CellKernel& choose_kernel(const BinPlan& bp, int b, int n, int n_cu)
{
    if (bp.latency[b] && n < bp.latency_below[b] * n_cu) return *bp.latency[b];
    return bp.lazy[b] ? *bp.lazy[b] : *bp.kernel[b];
}
inline bool is_lazy_sd(const CellKernel& k) { return k.family == CellFamily::wave_lz || k.family == CellFamily::pair_lz; }

}  // namespace ipc
