// shs_legacy_ext.hip -- the legacy kernels compiled with the extended shading models: Toon, Gooch,
// Oren-Nayar and the normal / depth visualisers (cpp-folders/src/hello-3d-primitives/
// hello_pipeline_{toon,gooch,oren_nayar}_shading.cpp, hello_pipeline_normal_zbuffer_debug.cpp), plus
// k_legacy_fs_sample (shs_legacy_shade_samples).
//
// The same source as shs_legacy.hip, in namespace shs_dev::ext / shs_internal::ext.  A translation unit
// of its own rather than a template parameter: the raster and group kernels sit at their register caps,
// and instantiations of one template in one compilation move each other's allocation; this way the
// kernels of a Flat .. Blinn-Phong batch are compiled from exactly the text they had before.
#define SHS_LEGACY_EXT 1
#include "shs_legacy.hip"
