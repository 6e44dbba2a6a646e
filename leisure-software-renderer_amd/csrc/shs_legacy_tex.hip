// shs_legacy_tex.hip -- the legacy kernels compiled with the texture-mapping pipeline, SHS_SHADING_TEXTURED
// (cpp-folders/src/hello-3d-primitives/hello_pipeline_texture_mapping.cpp:66-116, 205-294, and
// sample_nearest, hello-shs-renderer/shs_renderer.hpp:367-377), plus k_legacy_sample_nearest
// (shs_legacy_sample_nearest).
//
// The same source as shs_legacy.hip, in namespace shs_dev::tex / shs_internal::tex, with the extended
// shading models as well (a batch may mix them with model 9).  A third translation unit, not the second
// one growing: the textured pipeline changes the depth every pair test computes and widens the record, so
// in shs_legacy_ext.hip it would have changed the code -- and moved the registers -- of the Toon .. depth
// visualiser batches too; this way both earlier compilations keep the text they had.
#define SHS_LEGACY_EXT 1
#define SHS_LEGACY_TEX 1
#include "shs_legacy.hip"
