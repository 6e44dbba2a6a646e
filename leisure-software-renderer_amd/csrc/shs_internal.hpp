// shs_internal.hpp -- kernel launch wrappers shared between shs_legacy.hip and shs_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "shs_device.hpp"

namespace shs_internal {
hipError_t launch_setup(const shs_dev::FrameParams &fp, const shs_dev::FrameBuffers &fb, const shs_dev::KArgDraws &ka,
                        hipStream_t s);
hipError_t launch_ghost(const shs_dev::FrameParams &fp, const shs_dev::FrameBuffers &fb, hipStream_t s);
hipError_t launch_raster(const shs_dev::FrameParams &fp, const shs_dev::FrameBuffers &fb, const shs_dev::KArgDraws &ka,
                         int grid, hipStream_t s);
// k_pipe: batch k - 1's raster (fpR / fbR, grid = its persistent raster grid) and batch k's setup in one launch
hipError_t launch_pipe(const shs_dev::FrameParams &fpR, const shs_dev::FrameBuffers &fbR, int grid, const shs_dev::FrameParams &fpS,
                       const shs_dev::FrameBuffers &fbS, hipStream_t s);

// The compilation with the extended shading models (shs_legacy_ext.hip): the wrappers above hand a batch
// whose flags carry RF_EXT_MODELS to these.
namespace ext {
hipError_t launch_setup(const shs_dev::FrameParams &fp, const shs_dev::FrameBuffers &fb, const shs_dev::KArgDraws &ka,
                        hipStream_t s);
hipError_t launch_raster(const shs_dev::FrameParams &fp, const shs_dev::FrameBuffers &fb, const shs_dev::KArgDraws &ka,
                         int grid, hipStream_t s);
hipError_t launch_pipe(const shs_dev::FrameParams &fpR, const shs_dev::FrameBuffers &fbR, int grid, const shs_dev::FrameParams &fpS,
                       const shs_dev::FrameBuffers &fbS, hipStream_t s);
// k_legacy_fs_sample: n samples of d's fragment shader (d.shading, d.light ..); in = n normal sums, n
// world positions (3 floats each) and n clip z, all on the device
hipError_t launch_fs_sample(const shs_dev::DrawGPU &d, int n, const float *in, uint32_t *rgba, float4 *prequant, hipStream_t s);
}  // namespace ext

// The compilation with the texture-mapping pipeline (shs_legacy_tex.hip): a batch whose flags carry
// RF_TEX_MODEL goes to these, its ghost list included.
namespace tex {
hipError_t launch_setup(const shs_dev::FrameParams &fp, const shs_dev::FrameBuffers &fb, const shs_dev::KArgDraws &ka,
                        hipStream_t s);
hipError_t launch_ghost(const shs_dev::FrameParams &fp, const shs_dev::FrameBuffers &fb, hipStream_t s);
hipError_t launch_raster(const shs_dev::FrameParams &fp, const shs_dev::FrameBuffers &fb, const shs_dev::KArgDraws &ka,
                         int grid, hipStream_t s);
hipError_t launch_pipe(const shs_dev::FrameParams &fpR, const shs_dev::FrameBuffers &fbR, int grid, const shs_dev::FrameParams &fpS,
                       const shs_dev::FrameBuffers &fbS, hipStream_t s);
// k_legacy_sample_nearest: n (u, v) pairs through the rasters' sampler; texels, uv, rgba, index on the device
hipError_t launch_sample_nearest(const uint32_t *texels, int tw, int th, int n, const float2 *uv, uint32_t *rgba, int32_t *index,
                                 hipStream_t s);
}  // namespace tex
}  // namespace shs_internal
