// Compile check of wsamd::BatchSearch's WSAMD_WITH_OPENCV overload against tests/cxx/opencv_stub (NOT OpenCV: the
// declarations the adapters use), so that the block a cv::Mat caller compiles goes through a compiler here.
// tests/test_batch_core.py compiles it with -fsyntax-only; nothing runs.
#define WSAMD_WITH_OPENCV
#include "stereo_reconstruction_amd/host/window_search.hpp"

std::vector<cv::Mat> batch_of_mats(wsamd::BatchSearch &batch, const std::vector<std::pair<cv::Mat, cv::Mat>> &pairs)
{
    const ws_params p = wsamd::BatchSearch::params(WS_VIEW_LEFT, 7, 0, 256, 1.0);
    return batch.run(p, pairs, true, 256);
}
