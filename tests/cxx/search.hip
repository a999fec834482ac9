// The search family through the HPX C++ layer, compiled by hipcc, under seq,
// par and par(task), on the whole vector and on the sub-range [begin() + 1,
// end()), against the std:: algorithms on a host copy: find / find_if /
// find_if_not, all_of / any_of / none_of, count / count_if, min_element /
// max_element / minmax_element, equal / mismatch.  100003 ints drawn from
// 1000 values (four blocks; every extreme is repeated, so the tie rules show).
//
//   a value, fn::greater_than<int>, std::less<>, std::greater<int>,
//   std::equal_to<>                        the library's own kernels
//   [] (x) { x % 7 == 3 }, a comparator on x & 0xff, a projection x / 4,
//   [] (a, b) { a / 2 == b / 2 }           device closures
#include <hpx/hpx.hpp>
#include <hpx/hpx_init.hpp>
#include <hpx/include/parallel_all_any_none.hpp>
#include <hpx/include/parallel_count.hpp>
#include <hpx/include/parallel_equal.hpp>
#include <hpx/include/parallel_find.hpp>
#include <hpx/include/parallel_minmax.hpp>
#include <hpx/include/parallel_mismatch.hpp>
#include <hpx/util/lightweight_test.hpp>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <iostream>
#include <iterator>
#include <random>
#include <type_traits>
#include <utility>
#include <vector>

namespace hip = hpx::compute::hip;
namespace ex = hpx::parallel::execution;
namespace fn = hpx::compute::hip::functional;
using dvec = hpx::compute::vector<int, hip::allocator<int>>;
using It = dvec::iterator;
using HIt = std::vector<int>::const_iterator;

dvec to_dev(std::vector<int> const& h, hip::target const& t) {
    dvec d(h.size(), hip::allocator<int>(t));
    hpx::parallel::copy(ex::par, h.begin(), h.end(), d.begin());
    return d;
}
std::vector<int> to_host(dvec const& d) {
    std::vector<int> h(d.size());
    hpx::parallel::copy(ex::par, d.begin(), d.end(), h.begin());
    return h;
}

template <typename R>
R value_of(R r) {
    return r;
}
template <typename R>
R value_of(hpx::future<R> f) {
    return f.get();
}

struct quarter {
    HPX_HOST_DEVICE int operator()(int x) const { return x / 4; }
};

// One range [f, l) of the device vector and [hf, hl) of its host copy.
template <typename Policy>
void test_range(Policy const& pol, It f, It l, HIt hf, HIt hl) {
    constexpr bool task = std::decay_t<Policy>::is_task;
    auto at = [&](It r) { return r - f; };
    auto hat = [&](HIt r) { return r - hf; };
    const int present = hf == hl ? 5 : *(hf + (hl - hf) / 2), absent = -7;
    auto mod7 = [] HPX_HOST_DEVICE(int x) { return x % 7 == 3; };
    auto never = [] HPX_HOST_DEVICE(int x) { return x < 0; };
    auto always = [] HPX_HOST_DEVICE(int x) { return x >= 0; };
    fn::greater_than<int> big{990};
    fn::less_than<int> all_below{1000};

    // find, find_if, find_if_not
    {
        auto c = hpx::parallel::find(pol, f, l, present);
        static_assert(std::is_same<decltype(c), std::conditional_t<task, hpx::future<It>, It>>::value, "find result");
        HPX_TEST_EQ(at(value_of(std::move(c))), hat(std::find(hf, hl, present)));
    }
    HPX_TEST_EQ(at(value_of(hpx::find(pol, f, l, absent))), hat(hl));
    HPX_TEST_EQ(at(value_of(hpx::parallel::find_if(pol, f, l, big))), hat(std::find_if(hf, hl, big)));
    HPX_TEST_EQ(at(value_of(hpx::parallel::find_if(pol, f, l, mod7))), hat(std::find_if(hf, hl, mod7)));
    HPX_TEST_EQ(at(value_of(hpx::find_if(pol, f, l, never))), hat(hl));
    HPX_TEST_EQ(at(value_of(hpx::parallel::find_if_not(pol, f, l, fn::less_than<int>{900}))),
                hat(std::find_if_not(hf, hl, fn::less_than<int>{900})));
    HPX_TEST_EQ(at(value_of(hpx::find_if_not(pol, f, l, mod7))), hat(std::find_if_not(hf, hl, mod7)));
    HPX_TEST_EQ(at(value_of(hpx::parallel::find_if_not(pol, f, l, always))), hat(hl));

    // all_of, any_of, none_of
    {
        auto c = hpx::parallel::any_of(pol, f, l, big);
        static_assert(std::is_same<decltype(c), std::conditional_t<task, hpx::future<bool>, bool>>::value, "any_of");
        HPX_TEST_EQ(value_of(std::move(c)), std::any_of(hf, hl, big));
    }
    HPX_TEST_EQ(value_of(hpx::parallel::any_of(pol, f, l, mod7)), std::any_of(hf, hl, mod7));
    HPX_TEST_EQ(value_of(hpx::any_of(pol, f, l, never)), std::any_of(hf, hl, never));
    HPX_TEST_EQ(value_of(hpx::parallel::all_of(pol, f, l, all_below)), std::all_of(hf, hl, all_below));
    HPX_TEST_EQ(value_of(hpx::parallel::all_of(pol, f, l, big)), std::all_of(hf, hl, big));
    HPX_TEST_EQ(value_of(hpx::all_of(pol, f, l, always)), std::all_of(hf, hl, always));
    HPX_TEST_EQ(value_of(hpx::parallel::all_of(pol, f, l, mod7)), std::all_of(hf, hl, mod7));
    HPX_TEST_EQ(value_of(hpx::parallel::none_of(pol, f, l, big)), std::none_of(hf, hl, big));
    HPX_TEST_EQ(value_of(hpx::none_of(pol, f, l, never)), std::none_of(hf, hl, never));
    HPX_TEST_EQ(value_of(hpx::parallel::none_of(pol, f, l, mod7)), std::none_of(hf, hl, mod7));

    // count, count_if
    {
        auto c = hpx::parallel::count(pol, f, l, present);
        using D = std::iterator_traits<It>::difference_type;
        static_assert(std::is_same<decltype(c), std::conditional_t<task, hpx::future<D>, D>>::value, "count result");
        HPX_TEST_EQ(value_of(std::move(c)), std::count(hf, hl, present));
    }
    HPX_TEST_EQ(value_of(hpx::count(pol, f, l, absent)), 0);
    HPX_TEST_EQ(value_of(hpx::parallel::count_if(pol, f, l, big)), std::count_if(hf, hl, big));
    HPX_TEST_EQ(value_of(hpx::count_if(pol, f, l, mod7)), std::count_if(hf, hl, mod7));

    // min_element, max_element, minmax_element: the first smallest, the first
    // largest, (the first smallest, the last largest) -- the std:: rules
    auto low_byte = [] HPX_HOST_DEVICE(int x, int y) { return (x & 0xff) < (y & 0xff); };
    auto by_quarter = [](int x, int y) { return x / 4 < y / 4; };
    {
        auto c = hpx::parallel::min_element(pol, f, l);
        static_assert(std::is_same<decltype(c), std::conditional_t<task, hpx::future<It>, It>>::value, "min_element");
        HPX_TEST_EQ(at(value_of(std::move(c))), hat(std::min_element(hf, hl)));
        auto m = hpx::parallel::minmax_element(pol, f, l);
        using R = std::pair<It, It>;
        static_assert(std::is_same<decltype(m), std::conditional_t<task, hpx::future<R>, R>>::value, "minmax_element");
        R r = value_of(std::move(m));
        auto e = std::minmax_element(hf, hl);
        HPX_TEST_EQ(at(r.first), hat(e.first));
        HPX_TEST_EQ(at(r.second), hat(e.second));
    }
    HPX_TEST_EQ(at(value_of(hpx::max_element(pol, f, l))), hat(std::max_element(hf, hl)));
    HPX_TEST_EQ(at(value_of(hpx::parallel::min_element(pol, f, l, std::greater<int>()))),
                hat(std::min_element(hf, hl, std::greater<int>())));
    HPX_TEST_EQ(at(value_of(hpx::parallel::max_element(pol, f, l, std::greater<int>()))),
                hat(std::max_element(hf, hl, std::greater<int>())));
    HPX_TEST_EQ(at(value_of(hpx::parallel::min_element(pol, f, l, low_byte))), hat(std::min_element(hf, hl, low_byte)));
    HPX_TEST_EQ(at(value_of(hpx::parallel::max_element(pol, f, l, low_byte))), hat(std::max_element(hf, hl, low_byte)));
    HPX_TEST_EQ(at(value_of(hpx::min_element(pol, f, l, std::less<>(), quarter{}))),
                hat(std::min_element(hf, hl, by_quarter)));
    {
        auto r = value_of(hpx::minmax_element(pol, f, l, std::greater<int>()));
        auto e = std::minmax_element(hf, hl, std::greater<int>());
        HPX_TEST_EQ(at(r.first), hat(e.first));
        HPX_TEST_EQ(at(r.second), hat(e.second));
        r = value_of(hpx::parallel::minmax_element(pol, f, l, low_byte));
        e = std::minmax_element(hf, hl, low_byte);
        HPX_TEST_EQ(at(r.first), hat(e.first));
        HPX_TEST_EQ(at(r.second), hat(e.second));
        r = value_of(hpx::parallel::minmax_element(pol, f, l, std::less<>(), quarter{}));
        e = std::minmax_element(hf, hl, by_quarter);
        HPX_TEST_EQ(at(r.first), hat(e.first));
        HPX_TEST_EQ(at(r.second), hat(e.second));
    }
}

// equal and mismatch of [f, l) against a copy that differs at `where` (none if
// where < 0), which starts at another offset from a 16-B boundary.
template <typename Policy>
void test_pair(Policy const& pol, hip::target const& t, It f, It l, std::vector<int> const& h, std::ptrdiff_t where) {
    constexpr bool task = std::decay_t<Policy>::is_task;
    const std::ptrdiff_t n = l - f;
    std::vector<int> h2(h.size() + 3, 0);
    std::copy(h.begin(), h.end(), h2.begin() + 3);
    if (where >= 0) h2[3 + where] ^= 1;  // the same x / 2, another value
    dvec d2 = to_dev(h2, t);
    It f2 = d2.begin() + 3, l2 = d2.end();
    const std::ptrdiff_t exp = where >= 0 ? where : n;
    auto halves = [] HPX_HOST_DEVICE(int x, int y) { return x / 2 == y / 2; };
    {
        auto c = hpx::parallel::mismatch(pol, f, l, f2);
        using R = std::pair<It, It>;
        static_assert(std::is_same<decltype(c), std::conditional_t<task, hpx::future<R>, R>>::value, "mismatch");
        R r = value_of(std::move(c));
        HPX_TEST_EQ(r.first - f, exp);
        HPX_TEST_EQ(r.second - f2, exp);
        auto e = hpx::parallel::equal(pol, f, l, f2);
        static_assert(std::is_same<decltype(e), std::conditional_t<task, hpx::future<bool>, bool>>::value, "equal");
        HPX_TEST_EQ(value_of(std::move(e)), where < 0);
    }
    HPX_TEST_EQ(value_of(hpx::mismatch(pol, f, l, f2, std::equal_to<int>())).first - f, exp);
    HPX_TEST_EQ(value_of(hpx::equal(pol, f, l, f2, std::equal_to<>())), where < 0);
    // a binary predicate closure: the planted difference keeps x / 2
    HPX_TEST_EQ(value_of(hpx::parallel::mismatch(pol, f, l, f2, halves)).second - f2, n);
    HPX_TEST_EQ(value_of(hpx::parallel::equal(pol, f, l, f2, halves)), true);
    // four iterators
    HPX_TEST_EQ(value_of(hpx::parallel::mismatch(pol, f, l, f2, l2)).first - f, exp);
    HPX_TEST_EQ(value_of(hpx::parallel::equal(pol, f, l, f2, l2)), where < 0);
    HPX_TEST_EQ(value_of(hpx::parallel::equal(pol, f, l, f2, l2, halves)), true);
    if (n > 10) {
        auto r = value_of(hpx::parallel::mismatch(pol, f, l, f2, f2 + 10));
        HPX_TEST_EQ(r.first - f, std::min<std::ptrdiff_t>(exp, 10));
        HPX_TEST_EQ(value_of(hpx::parallel::equal(pol, f, l, f2, l2 - 1)), false);
        HPX_TEST_EQ(value_of(hpx::parallel::equal(pol, f, l, f2, l2 - 1, halves)), false);
    }
}

template <typename Policy>
void test_policy(Policy const& pol, hip::target const& t, std::mt19937& gen) {
    std::vector<int> a(100003);
    for (auto& x : a) x = static_cast<int>(gen() % 1000);
    dvec d = to_dev(a, t);
    for (std::size_t off : {std::size_t(0), std::size_t(1)}) {
        test_range(pol, d.begin() + off, d.end(), a.cbegin() + off, a.cend());
        std::vector<int> h(a.begin() + off, a.end());
        for (std::ptrdiff_t where : {std::ptrdiff_t(-1), std::ptrdiff_t(0), std::ptrdiff_t(70001), std::ptrdiff_t(h.size() - 1)})
            test_pair(pol, t, d.begin() + off, d.end(), h, where);
    }
    // an empty range and one element
    test_range(pol, d.begin() + 5, d.begin() + 5, a.cbegin() + 5, a.cbegin() + 5);
    test_range(pol, d.begin() + 5, d.begin() + 6, a.cbegin() + 5, a.cbegin() + 6);
    test_pair(pol, t, d.begin() + 5, d.begin() + 5, std::vector<int>(), -1);
    // a constant range: first smallest = first largest = 0, last largest = n - 1
    dvec c = to_dev(std::vector<int>(40000, 7), t);
    std::vector<int> hc(40000, 7);
    test_range(pol, c.begin(), c.end(), hc.cbegin(), hc.cend());
    HPX_TEST(to_host(d) == a);  // no call wrote to its input
}

int hpx_main(int, char*[]) {
    std::mt19937 gen(20261020);
    hip::target t;
    test_policy(ex::seq, t, gen);
    test_policy(ex::par, t, gen);
    test_policy(ex::par(ex::task), t, gen);
    return hpx::finalize();
}

int main(int argc, char* argv[]) {
    HPX_TEST_EQ(hpx::init(argc, argv), 0);
    int errors = hpx::util::report_errors();
    if (!errors) std::cout << "search: all tests passed" << std::endl;
    return errors;
}
