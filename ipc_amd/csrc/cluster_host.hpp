// Host-driven cluster solve, one launch per phase: the dog-leg control flow of cluster_common.hpp::cluster_dogleg on
// the host over the grid kernels of cluster_se2.hpp / cluster_se3.hpp (T = PersistSe2 / PersistSe3, the same bindings
// PersistSolver<T> runs on).  The Levenberg-retry fallback of the device-resident solver, the IPC_CLUSTER_MODE=host
// path and the long-cell path: needs no co-residency of workgroups and carries damping (damped_solve).
#pragma once
#include <memory>

namespace ipc {

template <class T>
class ClusterSolver {
public:
    using Dev = typename T::Dev;
    double term_eps = 0.0;             // convergence shortcut of the trial loop (Se2View::term_eps)

    // Solve chain lo..hi (records `chain`) + the loops `members` (indices into the candidate
    // records; ids in from/to are global vertex ids), starting from the poses `src` ([T::kPoseRows][src_ld], global
    // indexing).  The optimised poses stay in result() (local indexing 0..hi-lo).
    // chi_host (optional): per-edge chi2, odometry lo..hi-1 first, then the loops in `members` order.
    hipError_t solve(hipStream_t st, const double* chain, int estride, const double* cand, int cstride,
                     const double* src, int src_ld, int lo, int hi, const std::vector<int>& members, const int* from,
                     const int* to, int iterations, ClusterOut& out, std::vector<double>* chi_host);
    PoseBlock result() const { return PoseBlock{T::pose_rows(dev_.X), dev_.ld}; }

    // ---- Ops of cluster_dogleg ----
    hipError_t evaluate_committed(double& chi) { return evaluate(dev_.X, dev_.e, dev_.le, chi); }
    hipError_t linearize(double& bb, double& bHb, double& hh, double& bh, int& info);
    hipError_t blend(double alpha, double& c, double& bma);
    hipError_t trial(double p, double q, double& newChi, bool& anyChanged);
    void commit() { T::exchange(dev_); }
    hipError_t max_edge_chi2(double& mx);
    hipError_t damped_solve(double lambda, bool& ok, double& hh, double& bh, double& bHh, double& hHh);
    bool allow_damping = true;          // Levenberg retry of a failed linear solve on the literal normal equations: banded + bordered store
                                        // (cluster_literal_band.hpp) where the loops form a band, dense up to kMaxDenseN unknowns otherwise
    static constexpr int kMaxDenseN = 24000;
    static constexpr int kD = T::kD;
    int literal_band_min_n = 3072;      // IPC_LITERAL_BAND_MIN_N: smaller systems keep the dense store (bit for bit as in rounds 3 - 5); < 0: never banded
    std::unique_ptr<LiteralBand> lband; bool lband_stale = true;
    void want_plain_solve(bool w) { want_plain_ = w; }
    bool want_plain_ = true;
    long literal_band_solves() const { return lband ? lband->solves : 0; }
    const LoopTables& tables() const { return tab_; }
    hipStream_t stream() const { return st_; }
    template <class St> void launch_literal_H(const St& S, double lambda)
    {
        T::literal_H(dim3((dev_.L + 1 + T::kLiteralBlock - 1) / T::kLiteralBlock), st_, dev_, S, lambda);
    }

private:
    DevBuf<double> d_H_; size_t capH_ = 0;       // dense system + factor of damped_solve
    Dev dev_{};
    hipStream_t st_ = nullptr;
    int nblk_ = 1;
    std::vector<double>* chi_host_ = nullptr;
    int capL_ = 0, capNl_ = 0;
    DevBuf<double> d_edge_, d_loop_, d_S_, d_partial_, d_scal_;
    DevBuf<int> d_int_;
    int* d_info_ = nullptr;             // inside d_scal_
    PinnedBuf<double> h_scal_;          // pinned [12] + info
    LoopTables tab_;

    hipError_t ensure(int L, int nl);
    hipError_t fetch(int n)
    {
        (void)n;                     // scalars [0, 12) and the solver's info word at [12] travel in one copy
        IPC_CL_CHK(hipMemcpyAsync(h_scal_, d_scal_, sizeof(double) * 13, hipMemcpyDeviceToHost, st_));
        return hipStreamSynchronize(st_);
    }
    void sum_partials(int K, int off)
    {
        hipLaunchKernelGGL(gk_sum, dim3(1), dim3(64), 0, st_, (const double*)dev_.partial, nblk_, K, dev_.scal, off);
    }
    hipError_t evaluate(const decltype(Dev::X)& Y, double* eo, double* leo, double& chi)
    {
        hipLaunchKernelGGL(T::k_eval, dim3(nblk_), dim3(kGB), 0, st_, dev_, Y, eo, leo);
        sum_partials(1, 7);
        IPC_CL_CHK(fetch(8));
        chi = h_scal_[7];
        return hipSuccess;
    }
};

template <class T>
hipError_t ClusterSolver<T>::ensure(int L, int nl)
{
    if (!d_scal_) {                                  // (the last thing the block creates: a failure part way runs it again)
        IPC_CL_CHK(h_scal_.alloc(16));
        IPC_CL_CHK(d_scal_.alloc(16));
        d_info_ = reinterpret_cast<int*>(d_scal_ + 12);
    }
    if (L > capL_ || nl > capNl_) {
        const int nL = std::max(L, capL_), nN = std::max(nl, capNl_);
        capL_ = capNl_ = 0;
        const size_t ld = (size_t)nL + 2, n = (size_t)T::kD * nN;
        IPC_CL_CHK(d_edge_.alloc(T::kEdgeDoubles * ld + ld + nN));
        IPC_CL_CHK(d_loop_.alloc(T::kLoopDoubles * (size_t)nN + 8));
        IPC_CL_CHK(d_S_.alloc(2 * (n + 1) * n));     // system + factor
        IPC_CL_CHK(d_partial_.alloc(4 * ((nL + nN + 1 + kGB) / kGB + 1)));
        IPC_CL_CHK(d_int_.alloc(LoopTables::capacity(nL, nN)));
        capL_ = nL; capNl_ = nN;
    }
    return hipSuccess;
}

template <class T>
hipError_t ClusterSolver<T>::linearize(double& bb, double& bHb, double& hh, double& bh, int& info)
{
    Dev& D = dev_;
    const dim3 grid(nblk_), block(kGB);
    const int L = D.L, nl = D.nl, ld = D.ld, n = T::kD * nl;
    hipLaunchKernelGGL(T::k_force, grid, block, 0, st_, D);
    hipLaunchKernelGGL(T::k_b, grid, block, 0, st_, D);
    sum_partials(1, 0);
    hipLaunchKernelGGL(T::k_bHb_psi, grid, block, 0, st_, D);
    sum_partials(1, 1);
    if (!want_plain_) {                              // cluster_dogleg: only b, b^T b and b^T H b are needed, a damped solve follows
        IPC_CL_CHK(hipGetLastError());
        IPC_CL_CHK(fetch(4));
        bb = h_scal_[0]; bHb = h_scal_[1]; hh = 0.0; bh = 0.0; info = 1;
        return hipSuccess;
    }
    hipLaunchKernelGGL(gk_scan, dim3(T::kNPS), dim3(1024), 0, st_, D.ps, T::kNPS, L, ld);
    hipLaunchKernelGGL(T::k_assemble, dim3((nl + 63) / 64, nl), dim3(64), 0, st_, D);
    IPC_CL_CHK(chol_solve_device(D.S, D.S + (size_t)(n + 1) * n, n, D.rhs, d_info_, st_));
    hipLaunchKernelGGL(T::k_nu, dim3((nl + 63) / 64), dim3(64), 0, st_, D);
    hipLaunchKernelGGL(T::k_events, dim3((L + 2 + kGB - 1) / kGB), block, 0, st_, D);
    hipLaunchKernelGGL(gk_scan, dim3(T::kNND), dim3(1024), 0, st_, D.nd, T::kNND, L, ld);
    hipLaunchKernelGGL(T::k_rho, grid, block, 0, st_, D);
    hipLaunchKernelGGL(gk_scan, dim3(T::kSC1), dim3(1024), 0, st_, D.sc, T::kSC1, L, ld);
    hipLaunchKernelGGL(T::k_term, grid, block, 0, st_, D);
    hipLaunchKernelGGL(gk_scan, dim3(T::kSC2), dim3(1024), 0, st_, D.sc + T::kSC1 * (size_t)ld, T::kSC2, L, ld);
    hipLaunchKernelGGL(T::k_h, grid, block, 0, st_, D);
    sum_partials(2, 2);
    IPC_CL_CHK(hipGetLastError());
    IPC_CL_CHK(fetch(4));
    std::memcpy(&info, h_scal_ + 12, sizeof(int));
    bb = h_scal_[0]; bHb = h_scal_[1]; hh = h_scal_[2]; bh = h_scal_[3];
    return hipSuccess;
}

template <class T>
hipError_t ClusterSolver<T>::damped_solve(double lambda, bool& ok, double& hh, double& bh, double& bHh, double& hHh)
{
    Dev& D = dev_;
    const int n = T::kD * D.L;
    ok = false;
    IPC_CL_CHK(hipMemsetAsync(d_info_, 0, sizeof(int), st_));
    bool banded = false;
    if (literal_band_min_n >= 0 && n >= literal_band_min_n)
        IPC_CL_CHK(literal_band_damped(*this, lambda, banded, D.sc, d_info_));   // (solution in the scan workspace: kD ld doubles)
    if (!banded) {
        if (n > kMaxDenseN) return hipSuccess;                   // (no band and too large for the dense store: the solve reports Fail)
        const size_t m = (size_t)(n + 1) * n;
        if (2 * m > capH_) {
            capH_ = 0;
            IPC_CL_CHK(d_H_.alloc(2 * m));
            capH_ = 2 * m;
        }
        IPC_CL_CHK(hipMemsetAsync(d_H_, 0, sizeof(double) * m, st_));
        launch_literal_H(DenseStore{d_H_, n, T::kD}, lambda);
        IPC_CL_CHK(chol_solve_device(d_H_, d_H_ + m, n, D.sc, d_info_, st_));
    }
    hipLaunchKernelGGL(T::k_h_from_dense, dim3(nblk_), dim3(kGB), 0, st_, D, (const double*)D.sc);
    sum_partials(2, 2);
    hipLaunchKernelGGL(T::k_quad_bh, dim3(nblk_), dim3(kGB), 0, st_, D);
    sum_partials(2, 4);
    IPC_CL_CHK(hipGetLastError());
    IPC_CL_CHK(fetch(6));
    int info;
    std::memcpy(&info, h_scal_ + 12, sizeof(int));
    hh = h_scal_[2]; bh = h_scal_[3]; bHh = h_scal_[4]; hHh = h_scal_[5];
    ok = info == 0 && hh == hh;
    IPC_CL_CHK(hipMemsetAsync(d_info_, 0, sizeof(int), st_));
    return hipSuccess;
}

template <class T>
hipError_t ClusterSolver<T>::blend(double alpha, double& c, double& bma)
{
    hipLaunchKernelGGL(T::k_blend, dim3(nblk_), dim3(kGB), 0, st_, dev_, alpha);
    sum_partials(2, 4);
    IPC_CL_CHK(fetch(6));
    c = h_scal_[4]; bma = h_scal_[5];
    return hipSuccess;
}

template <class T>
hipError_t ClusterSolver<T>::trial(double p, double q, double& newChi, bool& anyChanged)
{
    hipLaunchKernelGGL(T::k_update, dim3(nblk_), dim3(kGB), 0, st_, dev_, p, q);
    sum_partials(1, 6);
    IPC_CL_CHK(evaluate(dev_.Xn, dev_.en, dev_.len, newChi));
    anyChanged = h_scal_[6] != 0.0;
    return hipSuccess;
}

template <class T>
hipError_t ClusterSolver<T>::max_edge_chi2(double& mx_out)
{
    Dev& D = dev_;
    hipLaunchKernelGGL(T::k_chi_edges, dim3(nblk_), dim3(kGB), 0, st_, D);
    IPC_CL_CHK(hipGetLastError());
    std::vector<double> local;
    std::vector<double>& chi = chi_host_ ? *chi_host_ : local;
    chi.resize((size_t)D.L + D.nl);
    IPC_CL_CHK(hipMemcpyAsync(chi.data(), D.chi_edges, sizeof(double) * chi.size(), hipMemcpyDeviceToHost, st_));
    IPC_CL_CHK(hipStreamSynchronize(st_));
    double mx = 0.0;
    bool nan = false;
    for (double c : chi) { if (c != c) nan = true; else mx = std::max(mx, c); }
    mx_out = (nan && !(mx > 0.0)) ? std::nan("") : mx;      // (max over the edges that have a number: se2_cell.hpp)
    return hipSuccess;
}

template <class T>
hipError_t ClusterSolver<T>::solve(hipStream_t st, const double* chain, int estride, const double* cand, int cstride,
                                   const double* src, int src_ld, int lo, int hi, const std::vector<int>& members,
                                   const int* from, const int* to, int iterations, ClusterOut& out,
                                   std::vector<double>* chi_host)
{
    const int L = hi - lo, nl = (int)members.size();
    IPC_CL_CHK(ensure(L, nl));
    const int ld = L + 2;
    st_ = st; chi_host_ = chi_host;
    Dev& D = dev_;
    D.chain = chain; D.estride = estride; D.lo = lo; D.L = L; D.nl = nl; D.ld = ld;
    D.cand = cand; D.cstride = cstride;
    T::carve(D, d_edge_, d_loop_, ld, nl);
    D.S = d_S_; D.ldS = T::kD * nl + 1;
    D.partial = d_partial_; D.scal = d_scal_;
    tab_.build(lo, hi, members, from, to);
    lband_stale = true;
    IPC_CL_CHK(hipMemcpyAsync(d_int_, tab_.host.data(), sizeof(int) * tab_.size(), hipMemcpyHostToDevice, st));
    IPC_CL_CHK(hipStreamSynchronize(st));           // the host table is pageable and reused
    D.lfrom = tab_.lfrom(d_int_); D.lto = tab_.lto(d_int_); D.lcand = tab_.lcand(d_int_);
    D.adj_ptr = tab_.adj_ptr(d_int_); D.adj_item = tab_.adj_item(d_int_);
    D.ev_ptr = tab_.ev_ptr(d_int_); D.ev_item = tab_.ev_item(d_int_);
    IPC_CL_CHK(hipMemcpy2DAsync(T::pose_rows(D.X), sizeof(double) * ld, src + lo, sizeof(double) * src_ld, sizeof(double) * (L + 1),
                                T::kPoseRows, hipMemcpyDeviceToDevice, st));
    nblk_ = (L + nl + 1 + kGB - 1) / kGB;            // indices 0 .. L+nl
    IPC_CL_CHK(hipMemsetAsync(d_info_, 0, sizeof(int), st));
    return cluster_dogleg(*this, iterations, out, term_eps, tab_.L + tab_.nl, allow_damping);
}

}  // namespace ipc
