// hpx/include/parallel_reduce.hpp -- forwards to the HIP backend's algorithm layer
// (reduce, and as in the reference reduce_by_key).
#pragma once
#include <hpx/parallel/algorithms.hpp>
