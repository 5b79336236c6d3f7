// APM_HD: the qualifier of the functions that are plain C++ as well as HIP (tri_index.h,
// update_item.h): compiled into the kernels, into the host code and into the host tests.
#pragma once
#ifdef __HIPCC__
#define APM_HD __host__ __device__
#else
#define APM_HD
#endif
