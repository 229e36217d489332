// fused-operator kernels of degree 3: instantiates the variant dispatch of bp5_device.hpp for this degree
#include "bp5_device.hpp"
template int apply_degree_impl<3>(bp5_mf *, ApplyCall &, const double *, const double *, double *);
template int apply_components_degree_impl<3>(bp5_mf *, const double *, int, size_t, const double *, double *, uint32_t, uint32_t);
