// hornSchunck.hpp -- drop-in replacement for HornSchunckOF/hornSchunck.cpp.
//
// The reference's main.cpp does `#include "hornSchunck.cpp"` (main.cpp:8)
// and then
//     hornSchunck hs = hornSchunck(windowSize, maxIterations, alpha); // :97
//     hs.getFlow(imagePrev, imageNext, u, v);                         // :98
// Replace that include with `#include "hornSchunck.hpp"` and link
// -lhsflow: the class below has the reference's exact public surface
// (hornSchunck.cpp:8-17 fields and ctor, :19 getGradients, :43 getFlow),
// takes cv::Mat by value, honours ROI steps, and returns CV_64FC1 u, v
// (plotFlow.cpp:72-75 reads them with at<double>).  The numerics run on the
// MI355X through libhsflow.so; errors surface as cv::Exception (CV_Error),
// as they would from inside OpenCV.
//
// Compiled only where OpenCV is available (the reference's own dependency);
// the OpenCV-free layer it wraps is hsflow.hpp.
#pragma once

#if __has_include(<opencv2/core.hpp>)
#include <opencv2/core.hpp>

#include <cstring>
#include <vector>

#include "hsflow.hpp"

class hornSchunck {
  public:
    int windowSize, maxIterations;
    double alpha;

    hornSchunck(int inpWindowSize, int inpMaxIterations, double inpAlpha)
        : windowSize(inpWindowSize), maxIterations(inpMaxIterations), alpha(inpAlpha),
          impl_(inpWindowSize, inpMaxIterations, inpAlpha) {}

    void getGradients(cv::Mat imagePrev, cv::Mat imageNext, cv::Mat &gradX, cv::Mat &gradY,
                      cv::Mat &gradT) {
        cv::Mat ha, hb;  // converted copies for depths the ABI does not take
        const hsflow::ImageView a = as_view(imagePrev, ha), b = as_view(imageNext, hb);
        gradX.create(imagePrev.rows, imagePrev.cols, CV_64FC1);
        gradY.create(imagePrev.rows, imagePrev.cols, CV_64FC1);
        gradT.create(imagePrev.rows, imagePrev.cols, CV_64FC1);
        if (gradX.step != gradY.step || gradX.step != gradT.step)
            CV_Error(cv::Error::StsInternal, "gradient steps differ");
        try {
            impl_.getGradientsInto(a, b, gradX.data, gradY.data, gradT.data, HSFLOW_F64,
                                   gradX.step);
        } catch (const hsflow::Error &e) {
            CV_Error(cv::Error::StsError, e.what());
        }
    }

    void getFlow(cv::Mat imagePrev, cv::Mat imageNext, cv::Mat &u, cv::Mat &v) {
        sync_params();
        cv::Mat ha, hb;
        const hsflow::ImageView a = as_view(imagePrev, ha), b = as_view(imageNext, hb);
        // hornSchunck.cpp:49-50 and :72-73 assign MatExprs (Mat::zeros, then
        // uAvg - uUpdateConst) to u, v; OpenCV evaluates a MatExpr into the
        // destination through create(), so an existing CV_64FC1 buffer of the
        // right size is written in place (headers sharing it see the result)
        // and anything else is reallocated.  create() here does the same.
        u.create(imagePrev.rows, imagePrev.cols, CV_64FC1);
        v.create(imagePrev.rows, imagePrev.cols, CV_64FC1);
        if (u.step != v.step) CV_Error(cv::Error::StsInternal, "u/v steps differ");
        try {
            impl_.getFlowInto(a, b, u.data, v.data, HSFLOW_F64, u.step);
        } catch (const hsflow::Error &e) {
            CV_Error(cv::Error::StsError, e.what());
        }
    }

    // Sequence mode of the context behind this object (hsflow.h,
    // hsflow_ctx_set_temporal): the bidirectional and interpolating solves
    // made through it start from the flow predicted from the previous call.
    void setTemporal(bool on) { guarded([&] { impl_.setTemporal(on); }); }
    bool temporal() {
        bool on = false;
        guarded([&] { on = impl_.temporal(); });
        return on;
    }
    void resetTemporal() { guarded([&] { impl_.resetTemporal(); }); }

    // The last pyramid level the warped, bidirectional and interpolating solves
    // made through this object solve (hsflow.h, hsflow_ctx_set_finest_level);
    // 0, the default: the full frame.
    void setFinestLevel(int finest) { guarded([&] { impl_.setFinestLevel(finest); }); }
    int finestLevel() {
        int finest = 0;
        guarded([&] { finest = impl_.finestLevel(); });
        return finest;
    }

    // Flow projection for the interpolating calls made through this object
    // (hsflow.h, hsflow_ctx_set_projection); 0, the default: none.
    void setProjection(int projection) { guarded([&] { impl_.setProjection(projection); }); }
    int projection() {
        int projection = 0;
        guarded([&] { projection = impl_.projection(); });
        return projection;
    }

    // The fallback for a failed pair of the interpolating calls made through
    // this object (hsflow.h, hsflow_ctx_set_fallback); nullptr, the default:
    // none.  lastCut: 1 where the last such call found a cut, 0 where the pair
    // passed, -1 where there was none.
    void setFallback(const hsflow_fallback *fb) { guarded([&] { impl_.setFallback(fb); }); }
    hsflow::Fallback fallback() {
        hsflow::Fallback fb(HSFLOW_FALLBACK_OFF, 0.0f);
        guarded([&] { fb = impl_.fallback(); });
        return fb;
    }
    int lastCut() {
        int cut = -1;
        guarded([&] { cut = impl_.lastCut(); });
        return cut;
    }

    // The 4:2:0 frames at `times` between two 8-bit 4:2:0 frames in OpenCV's own
    // representation of them -- CV_8UC1 of rows * 3 / 2 x cols, continuous: what
    // cv::cvtColor(COLOR_BGR2YUV_I420) gives and COLOR_YUV2BGR_I420 / _NV12
    // takes -- in the same layout (hsflow.h, hsflow_flow_interp_yuv): no colour
    // conversion, the luma is the grey frame.  frames[k] is created like the
    // inputs.  The settings above apply.  projection -1: none, and with the
    // projection setting on the call throws; 0 or 1: that, whatever the setting
    // (hsflow_flow_interp_yuv_pj).  Two CV_16UC1 frames of the same shape are
    // frames of 16-bit samples (yuv420p10le .. p16le, P010 .. P016) and give
    // CV_16UC1 frames (hsflow_flow_interp_yuv16; projection -1 stands for 0).
    void getFrameInterpYuv(const cv::Mat &imagePrev, const cv::Mat &imageNext,
                           const std::vector<float> &times, int levels, int warps, int median,
                           std::vector<cv::Mat> &frames, int layout = HSFLOW_YUV_I420,
                           int projection = -1) {
        sync_params();
        if (imagePrev.empty() || imageNext.empty()) CV_Error(cv::Error::StsBadArg, "empty image");
        const bool wide = imagePrev.type() == CV_16UC1 && imageNext.type() == CV_16UC1;
        if (!wide && (imagePrev.type() != CV_8UC1 || imageNext.type() != CV_8UC1))
            CV_Error(cv::Error::StsBadArg, "a 4:2:0 frame is CV_8UC1 of rows * 3 / 2 x cols");
        if (imagePrev.rows != imageNext.rows || imagePrev.cols != imageNext.cols)
            CV_Error(cv::Error::StsBadArg, "Image sizes are different");
        const size_t dense = (size_t)imagePrev.cols * (wide ? 2 : 1);
        if (imagePrev.rows % 3 || imagePrev.step != dense || imageNext.step != dense)
            CV_Error(cv::Error::StsBadArg,
                     "a 4:2:0 frame is continuous and rows * 3 / 2 rows high");
        const int rows = imagePrev.rows / 3 * 2, cols = imagePrev.cols;
        if (wide) {  // CV_16UC1: 16-bit samples in and out (hsflow_flow_interp_yuv16)
            std::vector<std::vector<uint16_t>> packed16;
            guarded([&] {
                impl_.getFrameInterpYuv((const uint16_t *)imagePrev.data,
                                        (const uint16_t *)imageNext.data, layout, rows, cols,
                                        times, levels, warps, median, packed16, nullptr,
                                        projection);
            });
            frames.resize(packed16.size());
            for (size_t k = 0; k < packed16.size(); ++k) {
                frames[k].create(imagePrev.rows, cols, CV_16UC1);
                std::memcpy(frames[k].data, packed16[k].data(), packed16[k].size() * 2);
            }
            return;
        }
        std::vector<std::vector<uint8_t>> packed;
        guarded([&] {
            impl_.getFrameInterpYuv(imagePrev.data, imageNext.data, layout, rows, cols, times,
                                    levels, warps, median, packed, nullptr, projection);
        });
        frames.resize(packed.size());
        for (size_t k = 0; k < packed.size(); ++k) {
            frames[k].create(imagePrev.rows, cols, CV_8UC1);
            std::memcpy(frames[k].data, packed[k].data(), packed[k].size());
        }
    }

  private:
    hsflow::HornSchunck impl_;

    template <typename F> static void guarded(F f) {
        try {
            f();
        } catch (const hsflow::Error &e) {
            CV_Error(cv::Error::StsError, e.what());
        }
    }

    void sync_params() {  // the public fields may be edited between calls
        impl_.windowSize = windowSize;
        impl_.maxIterations = maxIterations;
        impl_.alpha = alpha;
    }
    // A view of m for the C ABI; depths the ABI does not take are converted
    // into `holder` first, exactly as hornSchunck.cpp:23-24 converts every
    // input with convertTo(CV_64FC1).
    static hsflow::ImageView as_view(const cv::Mat &m, cv::Mat &holder) {
        if (m.empty()) CV_Error(cv::Error::StsBadArg, "empty image");
        if (m.channels() != 1)
            CV_Error(cv::Error::StsBadArg, "hornSchunck expects single-channel images "
                                           "(main.cpp:11-26 converts BGR to gray first)");
        const cv::Mat *src = &m;
        int type;
        switch (m.depth()) {
        case CV_8U: type = HSFLOW_U8; break;
        case CV_16F: type = HSFLOW_F16; break;
        case CV_32F: type = HSFLOW_F32; break;
        case CV_64F: type = HSFLOW_F64; break;
        default:  // CV_8S, CV_16U, CV_16S, CV_32S
            m.convertTo(holder, CV_64FC1);
            src = &holder;
            type = HSFLOW_F64;
        }
        hsflow::ImageView v;
        v.data = src->data;
        v.rows = src->rows;
        v.cols = src->cols;
        v.step = src->step;
        v.type = type;
        return v;
    }
};

#endif  // __has_include(<opencv2/core.hpp>)
