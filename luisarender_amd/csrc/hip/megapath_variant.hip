// megapath_variant.hip — ONE instantiation of the megakernel (feature mask LR_VARIANT, see megapath_kernel.h) and its
// launch / occupancy entry points for the kernel table (lrhip_kernels.hip).  Compiled once per mask of variants.h into its own object so that
// the variants build in parallel.
#include <hip/hip_runtime.h>

#ifndef LR_VARIANT
#error "compile with -DLR_VARIANT=<feature mask>"
#endif
#include "kernel_forms.h"
// kFeatPadded: the generic sampler is PaddedSobol, at compile time (dev_shade.h: LR_SAMPLER_KIND_OF)
#if ((LR_VARIANT) & LR_FEAT_PADDED) && !defined(LR_ONLY_SAMPLER)
#define LR_ONLY_SAMPLER LR_SAMPLER_PADDED_SOBOL
#endif
#if (LR_VARIANT) & LR_FEAT_VPT// the volumetric megakernel
#include "megavpt_kernel.h"
#define LR_KERNEL megavpt_kernel
#elif (LR_VARIANT) & LR_FEAT_POOL// the path-pool scheduler (round 4)
#include "megapath_kernel.h"
#include "megapool_kernel.h"
#define LR_KERNEL megapool_kernel
#else
#include "megapath_kernel.h"
#define LR_KERNEL megapath_kernel
#endif
#define LR_CAT2(a, b) a##b
#define LR_CAT(a, b) LR_CAT2(a, b)

// kernel_forms.h: what the preprocessor derived for this mask is what the host derives for it
static_assert(LR_IS(LR_MASK_MAKES_CALLS) == lrd::forms::makes_calls(LR_VARIANT), "kernel_forms.h: LR_CALL, LR_TEX_LAMBDA_ATTR");
static_assert(LR_DEFAULT_LOBE_FORM == lrd::forms::lobe_form(LR_VARIANT), "kernel_forms.h: LR_LOBE_FORM");
static_assert(LR_DEFAULT_BYTE_TEXELS == lrd::forms::decodes_byte_texels(LR_VARIANT), "kernel_forms.h: LR_BYTE_TEXELS");
static_assert(LR_DEFAULT_TEX_WIDE_RECORD == lrd::forms::wide_texture_record(LR_VARIANT), "kernel_forms.h: LR_TEX_WIDE_RECORD");
static_assert(LR_DEFAULT_LIGHT_OUT_OF_LINE == lrd::forms::light_out_of_line(LR_VARIANT), "kernel_forms.h: LR_LIGHT_OUT_OF_LINE");
static_assert(LR_DEFAULT_ENV_TREE == lrd::forms::walks_env_tree(LR_VARIANT), "kernel_forms.h: LR_ENV_TREE");
static_assert(LR_DEFAULT_NEST == lrd::forms::nests_closures(LR_VARIANT), "kernel_forms.h: LR_NEST");
static_assert(LR_DEFAULT_STRAIGHT_TAIL == lrd::forms::straight_tail(LR_VARIANT), "kernel_forms.h: LR_STRAIGHT_TAIL");
static_assert(LR_DEFAULT_LEAF_TAIL_ONE_COMPARE == lrd::forms::leaf_tail_one_compare(LR_VARIANT), "kernel_forms.h: LR_LEAF_TAIL_ONE_COMPARE");
static_assert(LR_DEFAULT_LIGHT_RECORDS == lrd::forms::light_records(LR_VARIANT), "kernel_forms.h: LR_LIGHT_RECORDS");

namespace lrd {
template __global__ void LR_KERNEL<LR_VARIANT>(DScenePtr, RenderArgs);
}

// `device_scene`: the lrd::DScene record in device memory (lrhip_render copies it there ahead of every launch).  `lds_bytes`: dynamic LDS per
// block -- the wave's tiles of the enabled AOV channels for the kFeatAov kernels (variants.h: LR_AOV_LIST), 0 for every other kernel
extern "C" hipError_t LR_CAT(lrhip_variant_launch_, LR_VARIANT)(unsigned blocks, hipStream_t stream, const lrd::DScene *device_scene,
                                                               const lrd::RenderArgs *args, unsigned lds_bytes) {
    hipLaunchKernelGGL(lrd::LR_KERNEL<LR_VARIANT>, dim3(blocks), dim3(lrd::kBlockThreads), lds_bytes, stream,
                       (lrd::DScenePtr)device_scene, *args);
    return hipGetLastError();
}

extern "C" hipError_t LR_CAT(lrhip_variant_occupancy_, LR_VARIANT)(int *blocks_per_cu, unsigned lds_bytes) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, lrd::LR_KERNEL<LR_VARIANT>, lrd::kBlockThreads, lds_bytes);
}
