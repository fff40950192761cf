// api_occlusion.hip — C ABI of the instance pipeline, part 5 of 6: the occlusion-culling extension (not reference behaviour).
// Depth pyramid builds, and mip_run_occluded: run_frame (api_frame.hip) with the occluded frame kernel in the frame kernel's
// place, so that outputs, host copies, frame slots and the per-triangle stage behind it are mip_run's own.
// The kernels (occlusion_kernel.hpp) are instantiated here and only here.
#include "context.hpp"
#include "occlusion_kernel.hpp"

namespace mip_host {
namespace {

// Levels, sizes and offsets of the pyramid of a W x H image (sides in 1 .. MIP_MAX_DEPTH_EXTENT).
struct PyramidLayout {
  uint32_t levels = 0;
  uint32_t w[16] = {0}, h[16] = {0};
  unsigned long long off[16] = {0};
  unsigned long long floats = 0;
};
PyramidLayout pyramid_layout(uint32_t width, uint32_t height) {
  PyramidLayout l;
  l.levels = mip::pyramid_levels(width, height);
  for (uint32_t k = 0; k < l.levels; ++k) {
    l.w[k] = mip::pyramid_level_extent(width, k);
    l.h[k] = mip::pyramid_level_extent(height, k);
    l.off[k] = l.floats;
    l.floats += (unsigned long long)l.w[k] * l.h[k];
  }
  return l;
}
static_assert(mip::pyramid_levels(MIP_MAX_DEPTH_EXTENT, MIP_MAX_DEPTH_EXTENT) <= 16, "level arrays");
static_assert(mip::kMaxDepthExtent == MIP_MAX_DEPTH_EXTENT && mip::kDepthUnorm16 == MIP_DEPTH_UNORM16 && mip::kDepthFloat32 == MIP_DEPTH_FLOAT32,
              "occlusion_kernel.hpp restates the header");

bool extent_ok(uint32_t width, uint32_t height) {
  return width >= 1u && height >= 1u && width <= MIP_MAX_DEPTH_EXTENT && height <= MIP_MAX_DEPTH_EXTENT;
}

}  // namespace

int32_t launch_occluded_frame(MipContext* ctx, const MipOcclusion* occ, mip::KernelArgs& a, const mip::LaunchPlan& plan, hipStream_t stream) {
  mip::OcclusionArgs oa{};
  oa.k = a;
  oa.k.first_mover_rule = 0;
  oa.pyramid = static_cast<const float*>(occ->pyramid);
  oa.candidates = occ->candidates;
  oa.occluded_bitmap = occ->occluded_bitmap;
  oa.candidates_xor = (occ->flags & MIP_OCC_CANDIDATES_INVERTED) ? ~0u : 0u;
  oa.width = occ->width;
  oa.height = occ->height;
  std::memcpy(oa.pv, occ->pv, sizeof oa.pv);
  void* params[] = {&oa};
  const void* fn = plan.general ? (const void*)mip::mip_occluded_frame_kernel<true> : (const void*)mip::mip_occluded_frame_kernel<false>;
  MIP_HIP(ctx, hipLaunchKernel(fn, dim3(plan.n_tiles), dim3(mip::kTile), params, 0, stream));
  MIP_HIP(ctx, hipGetLastError());
  return MIP_OK;
}

}  // namespace mip_host

using namespace mip_host;

extern "C" {

uint64_t mip_depth_pyramid_bytes(uint32_t width, uint32_t height) {
  if (!extent_ok(width, height)) return 0;
  return pyramid_layout(width, height).floats * 4ull;
}

int32_t mip_build_depth_pyramid(MipContext* ctx, const void* depth, uint32_t width, uint32_t height, uint32_t row_pitch_bytes,
                                uint32_t format, void* pyramid, int32_t async) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (!depth || !pyramid) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "depth/pyramid is NULL");
  if (!extent_ok(width, height))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "depth extent %ux%u outside 1..%u", width, height, (unsigned)MIP_MAX_DEPTH_EXTENT);
  if (format != MIP_DEPTH_UNORM16 && format != MIP_DEPTH_FLOAT32) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown depth format %u", format);
  const uint32_t elem = format == MIP_DEPTH_UNORM16 ? 2u : 4u;
  if (row_pitch_bytes % elem != 0u || (uint64_t)row_pitch_bytes < (uint64_t)width * elem)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "row pitch %u is not a multiple of %u bytes of at least %u pixels", row_pitch_bytes, elem, width);
  if ((uintptr_t)depth % elem != 0u || (uintptr_t)pyramid % 4u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "depth/pyramid is not aligned to its element");
  if (int32_t rc = bind_device(ctx)) return rc;
  // the stream of the slot the next frame will use: that frame is ordered after this build without a wait
  MipContext::FrameSlot& sl = ctx->slots[ctx->next_slot];
  if (!sl.d_pyramid_counter) {
    MIP_HIP(ctx, hipMalloc(&sl.d_pyramid_counter, 4));
    MIP_HIP(ctx, hipMemsetAsync(sl.d_pyramid_counter, 0, 4, sl.stream));
  }
  const PyramidLayout l = pyramid_layout(width, height);
  mip::PyramidArgs a{};
  a.depth = static_cast<const unsigned char*>(depth);
  a.pyramid = static_cast<float*>(pyramid);
  a.counter = sl.d_pyramid_counter;
  a.pitch = row_pitch_bytes;
  a.width = width;
  a.height = height;
  a.format = format;
  a.blocks_x = (width + mip::kPyramidBlock - 1u) / mip::kPyramidBlock;
  a.blocks = a.blocks_x * ((height + mip::kPyramidBlock - 1u) / mip::kPyramidBlock);
  a.levels = l.levels;
  a.vec = ((uintptr_t)depth % 16u == 0u && row_pitch_bytes % 16u == 0u) ? 1u : 0u;
  for (uint32_t k = 0; k < 16; ++k) {
    a.level_w[k] = l.w[k];
    a.level_h[k] = l.h[k];
    a.level_off[k] = l.off[k];
  }
  void* params[] = {&a};
  MIP_HIP(ctx, hipLaunchKernel((const void*)mip::mip_depth_pyramid_kernel, dim3(a.blocks), dim3(256), params, 0, sl.stream));
  MIP_HIP(ctx, hipGetLastError());
  return finish(ctx, sl.stream, async != 0);
}

int32_t mip_run_occluded(MipContext* ctx, const MipFrame* frame, const MipOcclusion* occ, const MipOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (!frame || !occ || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frame/occlusion/out is NULL");
  if (occ->struct_size != sizeof(MipOcclusion))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipOcclusion.struct_size %u != %zu", occ->struct_size, sizeof(MipOcclusion));
  if (!extent_ok(occ->width, occ->height))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "depth extent %ux%u outside 1..%u", occ->width, occ->height, (unsigned)MIP_MAX_DEPTH_EXTENT);
  if (occ->flags & ~MIP_OCC_CANDIDATES_INVERTED) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipOcclusion flags 0x%x", occ->flags);
  if (!occ->pyramid) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "pyramid is NULL");
  if ((occ->flags & MIP_OCC_CANDIDATES_INVERTED) && !occ->candidates)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MIP_OCC_CANDIDATES_INVERTED needs a candidate bitmap");
  if ((occ->candidates || occ->occluded_bitmap) && !(out->flags & MIP_OUT_DEVICE))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "candidates / occluded_bitmap need MIP_OUT_DEVICE");
  if (out->flags & (MIP_OUT_WIRE | MIP_OUT_WIRE_PACKED)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_run_occluded emits 20-byte commands only");
  return run_frame(ctx, frame, out, false, nullptr, occ);
}

}  // extern "C"
