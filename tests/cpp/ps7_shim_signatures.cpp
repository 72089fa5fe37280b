// Compile-time check that the shim's moments:: and matching:: have EXACTLY the types ps7_cpp/include/Moments.h and
// Matching.h declare, and that plotConfusionMatrix's default argument works.  Compiled by tests/test_ps7_shim.py; it
// has no run time.
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "introtocomputervision_amd/shim/micv_shim.hpp"
#include "introtocomputervision_amd/shim/micv_viz.hpp"

using micv_shim::Mat;

#define IS(f, ...) static_assert(std::is_same<decltype(&f), __VA_ARGS__>::value, #f " does not have the reference's type")

// Moments.h:9-12
IS(moments::centralMoment,
   std::vector<std::pair<float, float>> (*)(const Mat &, const std::vector<std::pair<int, int>> &));
// Matching.h:7, 12-16, 20-22
IS(matching::naiveConfusionMatrix, void (*)(const Mat &, const Mat &, Mat &));
IS(matching::confusionMatrix, void (*)(const Mat &, const Mat &, const Mat &, const size_t, std::vector<Mat> &));
IS(matching::plotConfusionMatrix, void (*)(const Mat &, const std::string &, const std::string &));
// the NORM_INF restatement the demo uses in place of cv::normalize
IS(micv_viz::normalize_inf_f32, Mat (*)(const Mat &));

inline void defaults(const Mat &c) { matching::plotConfusionMatrix(c, "title"); }
