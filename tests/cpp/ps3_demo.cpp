// runProblem1a, runProblem1bc, runProblem2 and runExtraCredit of ps3 (ProblemSets/ps3_cpp/src/Solution.cpp) on the
// shim: the `points:` files and the `mersenne_seed` of a ps3.yaml-format file, every matrix printed in the shape of
// the reference's log (five digits, columns of 13) and once more as hex floats ("hex <name> ...") for
// tests/test_ps3_shim.py.  The images only give the driver their size; here it is an argument.
//   ps3_demo <ps3.yaml> <dir with the point files> <image rows> <image cols>
#include <cstdio>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

#include "../../introtocomputervision_amd/shim/micv_config.hpp"
#include "../../introtocomputervision_amd/shim/micv_geom.hpp"

using micv_shim::Mat;

static void print_mat(const char *title, const Mat &m) {
    std::cout << title << "\n[" << std::setprecision(5);
    for (int y = 0; y < m.rows; y++) {
        std::cout << (y == 0 ? " " : "  ");
        for (int x = 0; x < m.cols; x++) std::cout << std::left << std::setw(13) << m.ptr<float>(y)[x];
        std::cout << (y < m.rows - 1 ? "\n" : " ");
    }
    std::cout << "]" << std::endl;
}
static void print_hex(const char *name, const Mat &m) {
    std::printf("hex %s", name);
    for (int y = 0; y < m.rows; y++)
        for (int x = 0; x < m.cols; x++) std::printf(" %a", (double)m.ptr<float>(y)[x]);
    std::printf("\n");
    std::fflush(stdout);
}
static Mat to_mat(const micv_config::PointSet &p) {
    Mat m(p.dims, p.n, micv_shim::F32);
    for (int d = 0; d < p.dims; d++)
        for (int i = 0; i < p.n; i++) m.ptr<float>(d)[i] = p.data[(size_t)d * p.n + i];
    return m;
}
static Mat reshape(const Mat &col, int rows, int cols) {
    Mat m(rows, cols, micv_shim::F32);
    for (int i = 0; i < rows * cols; i++) m.ptr<float>(i / cols)[i % cols] = col.ptr<float>(i)[0];
    return m;
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const micv_config::Node cfg = micv_config::Node::load(argv[1]);
    const std::string dir = argv[2];
    const int rows = std::stoi(argv[3]), cols = std::stoi(argv[4]);
    const micv_config::PS3Points pts(cfg.child("points"), [&](const std::string &p) {
        return dir + "/" + p.substr(p.find_last_of('/') + 1);
    });
    if (!pts.ok) return 3;
    const Mat picA = to_mat(pts.picA), picB = to_mat(pts.picB), picANorm = to_mat(pts.picANorm),
              pts3D = to_mat(pts.pts3D), pts3DNorm = to_mat(pts.pts3DNorm);

    // problem 1a
    const Mat ls = reshape(calib::solveLeastSquares(picANorm, pts3DNorm), 3, 4);
    print_mat("Calibration parameters (using normal least squares):", ls);
    print_hex("M_ls", ls);
    const Mat svd = reshape(calib::solveSVD(picANorm, pts3DNorm), 3, 4);
    print_mat("Calibration parameters (using singular value decomposition):", svd);
    print_hex("M_svd", svd);

    // problems 1b and 1c
    const auto seed = micv_config::mersenne_seed(cfg);
    const micv_geom::Trials tr = micv_geom::calibrationTrials(picB, pts3D, *seed);
    std::cout << "All computed residuals:\n[" << std::setprecision(16);
    for (size_t i = 0; i < tr.residuals.size(); i++)
        std::cout << tr.residuals[i] << (i + 1 == tr.residuals.size() ? "]\n" : (i % 3 == 2 ? ";\n " : ", "));
    std::printf("hex residuals");
    for (double r : tr.residuals) std::printf(" %a", r);
    std::printf("\n");
    std::fflush(stdout);
    std::cout << "Minimum residual: " << std::setprecision(6) << tr.minResidual
              << "\nFound with constraint size: " << tr.constraintSize << std::endl;
    if (tr.params.empty()) return 4;  // no trial with a finite residual
    print_mat("Computed parameters:", tr.params);
    print_hex("M_best", tr.params);
    const Mat center = micv_geom::cameraCenter(tr.params);
    print_mat("Center of camera:", center);
    print_hex("center", center);

    // problem 2
    const Mat fEst = reshape(fundamental::solveLeastSquares(picA, picB), 3, 3);
    print_mat("Fundamental matrix estimate:", fEst);
    print_hex("F_est", fEst);
    const Mat fMat = fundamental::rankReduce(fEst);
    print_mat("Fundamental matrix with rank = 2", fMat);
    print_hex("F_rank2", fMat);
    print_hex("ends_2_a", micv_geom::epipolarEndpoints(fMat, picB, 0, rows, cols));
    print_hex("ends_2_b", micv_geom::epipolarEndpoints(fMat, picA, 1, rows, cols));

    // extra credit
    const micv_geom::Normalized nf = micv_geom::normalizedFundamental(picA, picB);
    print_mat("Transform matrix T_a:", nf.transformA);
    print_hex("T_a", nf.transformA);
    print_mat("Transform matrix T_b:", nf.transformB);
    print_hex("T_b", nf.transformB);
    print_mat("Fundamental matrix F_Hat:", nf.FHat);
    print_hex("F_hat", nf.FHat);
    print_mat("\"Better\" fundamental matrix F:", nf.F);
    print_hex("F_better", nf.F);
    print_hex("ends_e_a", micv_geom::epipolarEndpoints(nf.F, picB, 0, rows, cols));
    print_hex("ends_e_b", micv_geom::epipolarEndpoints(nf.F, picA, 1, rows, cols));
    return 0;
}
