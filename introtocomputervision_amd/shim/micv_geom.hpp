// micv_geom.hpp -- calib:: and fundamental:: of the reference's ps3 library (ProblemSets/ps3_cpp/include/
// Calibration.h, Fundamental.h) over libmicv.so's "ps3: geometry" entry points, plus the pieces of the driver
// (ps3_cpp/src/Solution.cpp) that are arithmetic: the trial loop of problem 1b/1c, the camera centre, the normalised
// chain of the extra credit and the end points of the epipolar lines.  Points are 2 x n / 3 x n CV_32F matrices as the
// reference keeps them; the C ABI wants rows, so every call transposes on the way in.
//
// With -DMICV_SHIM_WITH_EIGEN the Eigen::MatrixXf overloads of the two headers are declared as well (they copy
// through the Mat ones).
#pragma once

#include <memory>
#include <random>
#include <vector>

#include "micv_shim.hpp"

#ifdef MICV_SHIM_WITH_EIGEN
#include <Eigen/Dense>
#endif

namespace micv_geom {
using micv_shim::Mat;

// d x n CV_32F -> n rows of d floats
inline std::vector<float> rows_of(const Mat &m, int d, const char *what) {
    micv_shim::require(m.type() == micv_shim::F32 && m.rows == d && m.cols >= 1, what);
    std::vector<float> out((size_t)m.cols * d);
    for (int r = 0; r < d; r++)
        for (int c = 0; c < m.cols; c++) out[(size_t)c * d + r] = m.ptr<float>(r)[c];
    return out;
}
inline Mat column(const std::vector<float> &v) {
    Mat m((int)v.size(), 1, micv_shim::F32);
    for (size_t i = 0; i < v.size(); i++) m.ptr<float>((int)i)[0] = v[i];
    return m;
}
inline Mat mat3(const float *v, int rows = 3, int cols = 3) {
    Mat m(rows, cols, micv_shim::F32);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) m.ptr<float>(r)[c] = v[r * cols + c];
    return m;
}
inline std::vector<float> flat(const Mat &m, int count, const char *what) {
    micv_shim::require(m.type() == micv_shim::F32 && m.rows * m.cols == count, what);
    std::vector<float> out;
    for (int r = 0; r < m.rows; r++)
        for (int c = 0; c < m.cols; c++) out.push_back(m.ptr<float>(r)[c]);
    return out;
}

// The trial loop of Solution.cpp:243-318 as one launch: for each constraint set size `iters` trials on the first
// `size` entries of a fresh shuffle, the next `tests` entries as test points.
struct Trials {
    std::vector<double> residuals;  // [iters][sizes], the layout the driver prints
    double minResidual = 0;
    size_t constraintSize = 0;
    Mat params;  // 3 x 4, empty when no trial had a finite residual
};
inline Trials calibrationTrials(const Mat &pts2d, const Mat &pts3d, std::seed_seq &seed,
                                const std::vector<size_t> &sizes = {8, 12, 16}, size_t iters = 10, size_t tests = 4,
                                unsigned flags = 0) {
    const std::vector<float> p2 = rows_of(pts2d, 2, "calibrationTrials: 2 x n CV_32F expected"),
                             p3 = rows_of(pts3d, 3, "calibrationTrials: 3 x n CV_32F expected");
    const int n = pts2d.cols;
    micv_shim::require(pts3d.cols == n && !sizes.empty() && iters >= 1, "calibrationTrials: bad argument");
    std::vector<uint32_t> words;
    seed.param(std::back_inserter(words));
    micv_ransac_rng *rng = nullptr;
    micv_shim::check(micv_ransac_rng_create(words.data(), (int)words.size(), &rng));
    std::unique_ptr<micv_ransac_rng, void (*)(micv_ransac_rng *)> guard(rng, micv_ransac_rng_destroy);
    size_t kmax = 0;
    for (size_t s : sizes) kmax = std::max(kmax, s);
    const int T = (int)(sizes.size() * iters), stride = (int)(kmax + tests);
    std::vector<int32_t> perms((size_t)T * n), idx((size_t)T * stride, 0), kc(T);
    micv_shim::check(micv_geom_trial_indices(rng, n, T, perms.data()));
    std::vector<int> groups(sizes.size(), (int)iters);
    for (int t = 0; t < T; t++) {
        kc[t] = (int32_t)sizes[t / iters];
        for (size_t i = 0; i < kc[t] + tests && i < (size_t)n; i++) idx[(size_t)t * stride + i] = perms[(size_t)t * n + i];
    }
    const size_t G = sizes.size();
    std::vector<float> M((size_t)T * 12), bM((G + 1) * 12);
    std::vector<double> res(T), bres(G + 1);
    std::vector<int32_t> bidx(G + 1);
    micv_shim::check(micv_calib_ls_trials_host(micv_shim::context(), p2.data(), p3.data(), n, idx.data(), stride,
                                               (int)kmax, (int)tests, T, kc.data(), groups.data(), (int)G, flags,
                                               M.data(), res.data(), bidx.data(), bres.data(), bM.data()));
    Trials out;
    out.residuals.resize(T);
    for (int t = 0; t < T; t++) out.residuals[(t % iters) * G + t / iters] = res[t];
    out.minResidual = bres[G];
    if (bidx[G] >= 0) {
        out.constraintSize = sizes[bidx[G] / iters];
        out.params = mat3(bM.data() + G * 12, 3, 4);
    }
    return out;
}

// -Q^-1 m4 of a 3 x 4 projection matrix -> 3 x 1.
inline Mat cameraCenter(const Mat &params, unsigned flags = 0) {
    const std::vector<float> m = flat(params, 12, "cameraCenter: 3 x 4 CV_32F expected");
    std::vector<float> c(3);
    micv_shim::check(micv_camera_center_host(micv_shim::context(), m.data(), 1, flags, c.data()));
    return column(c);
}

struct Normalized {
    Mat transformA, transformB, FHat, F;
};
inline Normalized normalizedFundamental(const Mat &pts2dA, const Mat &pts2dB, unsigned flags = 0) {
    const std::vector<float> a = rows_of(pts2dA, 2, "normalizedFundamental: 2 x n CV_32F expected"),
                             b = rows_of(pts2dB, 2, "normalizedFundamental: 2 x n CV_32F expected");
    micv_shim::require(pts2dA.cols == pts2dB.cols, "normalizedFundamental: point counts differ");
    float o[36];
    micv_shim::check(micv_fundamental_normalized_host(micv_shim::context(), a.data(), b.data(), pts2dA.cols, flags, o,
                                                      o + 9, o + 18, o + 27));
    return Normalized{mat3(o), mat3(o + 9), mat3(o + 18), mat3(o + 27)};
}

// The end points drawEpipolarLines computes (n x 6: P_iL, P_iR).  side 0: pts are image B's, the lines lie in image
// A ((p^T F)^T); side 1: pts are image A's, the lines lie in image B (F p).
inline Mat epipolarEndpoints(const Mat &fMat, const Mat &pts2d, int side, int rows, int cols, unsigned flags = 0) {
    const std::vector<float> F = flat(fMat, 9, "epipolarEndpoints: 3 x 3 CV_32F expected"),
                             p = rows_of(pts2d, 2, "epipolarEndpoints: 2 x n CV_32F expected");
    Mat out(pts2d.cols, 6, micv_shim::F32);
    micv_shim::check(micv_epipolar_endpoints_host(micv_shim::context(), F.data(), p.data(), pts2d.cols, side, rows, cols,
                                                  flags, out.ptr<float>()));
    return out;
}
}  // namespace micv_geom

namespace calib {  // ProblemSets/ps3_cpp/include/Calibration.h
using micv_shim::Mat;
inline Mat solveLeastSquares(const Mat &pts2d, const Mat &pts3d) {
    const std::vector<float> p2 = micv_geom::rows_of(pts2d, 2, "calib::solveLeastSquares: 2 x n CV_32F expected"),
                             p3 = micv_geom::rows_of(pts3d, 3, "calib::solveLeastSquares: 3 x n CV_32F expected");
    micv_shim::require(pts2d.cols == pts3d.cols, "calib::solveLeastSquares: point counts differ");
    std::vector<float> M(12);
    double residual;
    micv_shim::check(micv_calib_ls_trials_host(micv_shim::context(), p2.data(), p3.data(), pts2d.cols, nullptr, 0,
                                               pts2d.cols, 0, 1, nullptr, nullptr, 0, 0, M.data(), &residual, nullptr,
                                               nullptr, nullptr));
    return micv_geom::column(M);
}
inline Mat solveSVD(const Mat &pts2d, const Mat &pts3d) {
    const std::vector<float> p2 = micv_geom::rows_of(pts2d, 2, "calib::solveSVD: 2 x n CV_32F expected"),
                             p3 = micv_geom::rows_of(pts3d, 3, "calib::solveSVD: 3 x n CV_32F expected");
    micv_shim::require(pts2d.cols == pts3d.cols, "calib::solveSVD: point counts differ");
    std::vector<float> M(12);
    micv_shim::check(micv_calib_svd_host(micv_shim::context(), p2.data(), p3.data(), pts2d.cols, nullptr, 0, pts2d.cols,
                                         1, 0, M.data()));
    return micv_geom::column(M);
}
}  // namespace calib

namespace fundamental {  // ProblemSets/ps3_cpp/include/Fundamental.h
using micv_shim::Mat;
inline Mat solveLeastSquares(const Mat &pts2dA, const Mat &pts2dB) {
    const std::vector<float> a = micv_geom::rows_of(pts2dA, 2, "fundamental::solveLeastSquares: 2 x n CV_32F expected"),
                             b = micv_geom::rows_of(pts2dB, 2, "fundamental::solveLeastSquares: 2 x n CV_32F expected");
    micv_shim::require(pts2dA.cols == pts2dB.cols, "fundamental::solveLeastSquares: point counts differ");
    std::vector<float> F(9);
    micv_shim::check(micv_fundamental_ls_host(micv_shim::context(), a.data(), b.data(), pts2dA.cols, nullptr, 0,
                                              pts2dA.cols, 1, 0, F.data()));
    return micv_geom::column(F);
}
inline Mat rankReduce(const Mat &fMat) {
    const std::vector<float> F = micv_geom::flat(fMat, 9, "fundamental::rankReduce: 3 x 3 CV_32F expected");
    micv_shim::require(fMat.rows == 3, "fundamental::rankReduce: 3 x 3 CV_32F expected");
    float out[9];
    micv_shim::check(micv_fundamental_rank_reduce_host(micv_shim::context(), F.data(), 1, 0, out));
    return micv_geom::mat3(out);
}
}  // namespace fundamental

#ifdef MICV_SHIM_WITH_EIGEN
namespace micv_geom {
inline Mat from_eigen(const Eigen::MatrixXf &m) {
    Mat out((int)m.rows(), (int)m.cols(), micv_shim::F32);
    for (int r = 0; r < out.rows; r++)
        for (int c = 0; c < out.cols; c++) out.ptr<float>(r)[c] = m(r, c);
    return out;
}
inline Eigen::MatrixXf to_eigen(const Mat &m) {
    Eigen::MatrixXf out(m.rows, m.cols);
    for (int r = 0; r < m.rows; r++)
        for (int c = 0; c < m.cols; c++) out(r, c) = m.ptr<float>(r)[c];
    return out;
}
}  // namespace micv_geom
namespace calib {
inline Eigen::MatrixXf solveLeastSquares(const Eigen::MatrixXf &pts2d, const Eigen::MatrixXf &pts3d) {
    return micv_geom::to_eigen(solveLeastSquares(micv_geom::from_eigen(pts2d), micv_geom::from_eigen(pts3d)));
}
inline Eigen::MatrixXf solveSVD(const Eigen::MatrixXf &pts2d, const Eigen::MatrixXf &pts3d) {
    return micv_geom::to_eigen(solveSVD(micv_geom::from_eigen(pts2d), micv_geom::from_eigen(pts3d)));
}
}  // namespace calib
namespace fundamental {
inline Eigen::MatrixXf solveLeastSquares(const Eigen::MatrixXf &pts2dA, const Eigen::MatrixXf &pts2dB) {
    return micv_geom::to_eigen(solveLeastSquares(micv_geom::from_eigen(pts2dA), micv_geom::from_eigen(pts2dB)));
}
inline Eigen::MatrixXf rankReduce(const Eigen::MatrixXf &fMat) {
    return micv_geom::to_eigen(rankReduce(micv_geom::from_eigen(fMat)));
}
}  // namespace fundamental
#endif
