// hpx/include/parallel_algorithm.hpp -- forwards to the HIP backend's algorithm layer.
#pragma once
#include <hpx/parallel/algorithms.hpp>
#include <hpx/include/parallel_unique.hpp>
#include <hpx/include/parallel_all_any_none.hpp>
#include <hpx/include/parallel_count.hpp>
#include <hpx/include/parallel_equal.hpp>
#include <hpx/include/parallel_find.hpp>
#include <hpx/include/parallel_minmax.hpp>
#include <hpx/include/parallel_mismatch.hpp>
#include <hpx/include/parallel_set_operations.hpp>
#include <hpx/include/parallel_reverse.hpp>
#include <hpx/include/parallel_rotate.hpp>
#include <hpx/include/parallel_swap_ranges.hpp>
#include <hpx/include/parallel_replace.hpp>
#include <hpx/include/parallel_adjacent_difference.hpp>
