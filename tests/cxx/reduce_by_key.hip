// hpx::parallel::reduce_by_key (reduce_by_key.hpp:586) through the HPX C++
// layer, compiled by hipcc: the reference test's recipe restated -- runs of
// 1..256 equal keys, neighbouring runs with different keys, values in
// [-256, 256] -- run IN PLACE (keys_output == key_first, values_output ==
// values_first), under seq, par and par(task), against a sequential host
// fold:
//
//   std::equal_to + std::plus                 the library's own kernels
//   a comparator equating keys by k / 4       device closure
//   "take first" f(a, b) = a, "take last" f(a, b) = b
//                                             associative, non-commutative and
//                                             identity-free: each run's first
//                                             and last value
//   n == 0 and n == 1                         the ends of what was written
//
// usage: reduce_by_key [seed]
#include <hpx/hpx.hpp>
#include <hpx/hpx_init.hpp>
#include <hpx/include/parallel_reduce.hpp>
#include <hpx/util/lightweight_test.hpp>

#include <cstdint>
#include <cstdlib>
#include <functional>
#include <iostream>
#include <random>
#include <utility>
#include <vector>

namespace hip = hpx::compute::hip;
namespace ex = hpx::parallel::execution;
template <typename T>
using dvec = hpx::compute::vector<T, hip::allocator<T>>;

template <typename T>
std::vector<T> to_host(dvec<T> const& d) {
    std::vector<T> h(d.size());
    hpx::parallel::copy(ex::par, d.begin(), d.end(), h.begin());
    return h;
}
template <typename T>
dvec<T> to_dev(std::vector<T> const& h, hip::target const& t) {
    dvec<T> d(h.size(), hip::allocator<T>(t));
    hpx::parallel::copy(ex::par, h.begin(), h.end(), d.begin());
    return d;
}

struct quarter_equal {
    HPX_HOST_DEVICE bool operator()(int64_t a, int64_t b) const { return a / 4 == b / 4; }
};
struct take_first {
    HPX_HOST_DEVICE double operator()(double a, double) const { return a; }
};
struct take_last {
    HPX_HOST_DEVICE double operator()(double, double b) const { return b; }
};

// the sequential meaning: one (first key, left fold) per run
template <typename K, typename V, typename Comp, typename Func>
void host_reduce_by_key(std::vector<K> const& k, std::vector<V> const& v, Comp comp, Func func, std::vector<K>& ko,
                        std::vector<V>& vo) {
    ko.clear();
    vo.clear();
    for (std::size_t i = 0; i < k.size(); ++i) {
        if (i > 0 && comp(k[i - 1], k[i])) {
            vo.back() = func(vo.back(), v[i]);
        } else {
            ko.push_back(k[i]);
            vo.push_back(v[i]);
        }
    }
}

// runs of 1..256 keys; a new run's key differs from the one before it by at
// least 4, so the runs are the same under == and under k / 4 once the keys
// of a run are spread over one quarter (spread = true)
void make_input(std::mt19937_64& gen, std::size_t n, bool spread, std::vector<int64_t>& k, std::vector<double>& v) {
    k.resize(n);
    v.resize(n);
    int64_t key = int64_t(gen() % 1000) * 4;
    for (std::size_t i = 0; i < n;) {
        std::size_t len = 1 + gen() % 256;
        key += 4 * int64_t(1 + gen() % 5);
        for (std::size_t j = 0; j < len && i < n; ++j, ++i) {
            k[i] = spread ? key + int64_t(gen() % 4) : key;
            v[i] = double(int64_t(gen() % 513) - 256);
        }
    }
}

template <typename T>
void expect_prefix(std::vector<T> const& got, std::vector<T> const& exp, char const* what, std::size_t n) {
    for (std::size_t i = 0; i < exp.size(); ++i)
        if (!(got[i] == exp[i])) {
            std::cout << what << " n=" << n << ": first mismatch at " << i << std::endl;
            HPX_TEST(false);
            return;
        }
}

template <typename Policy, typename Comp, typename Func>
void run_in_place(Policy const& pol, hip::target const& t, std::vector<int64_t> const& k, std::vector<double> const& v,
                  Comp comp, Func func, char const* what) {
    std::vector<int64_t> ek;
    std::vector<double> ev;
    host_reduce_by_key(k, v, comp, func, ek, ev);
    auto dk = to_dev(k, t);
    auto dv = to_dev(v, t);
    std::pair<typename dvec<int64_t>::iterator, typename dvec<double>::iterator> r;
    if constexpr (std::decay_t<Policy>::is_task) {
        hpx::future<decltype(r)> f =
            hpx::parallel::reduce_by_key(pol, dk.begin(), dk.end(), dv.begin(), dk.begin(), dv.begin(), comp, func);
        r = f.get();
    } else {
        r = hpx::parallel::reduce_by_key(pol, dk.begin(), dk.end(), dv.begin(), dk.begin(), dv.begin(), comp, func);
    }
    HPX_TEST_EQ(std::size_t(r.first - dk.begin()), ek.size());
    HPX_TEST_EQ(std::size_t(r.second - dv.begin()), ek.size());
    if (std::size_t(r.first - dk.begin()) != ek.size()) {
        std::cout << what << " n=" << k.size() << ": run count" << std::endl;
        return;
    }
    expect_prefix(to_host(dk), ek, what, k.size());
    expect_prefix(to_host(dv), ev, what, k.size());
}

template <typename Policy>
void test_policy(Policy const& pol, hip::target const& t, std::mt19937_64& gen) {
    for (std::size_t n : {std::size_t(0), std::size_t(1), std::size_t(2), std::size_t(1000), std::size_t(8193),
                          std::size_t(100003), std::size_t(70) * 8192 + 5}) {
        std::vector<int64_t> k;
        std::vector<double> v;
        make_input(gen, n, false, k, v);
        run_in_place(pol, t, k, v, std::equal_to<int64_t>(), std::plus<double>(), "equal_to, plus");
        run_in_place(pol, t, k, v, std::equal_to<>(), take_first(), "equal_to, take first");
        run_in_place(pol, t, k, v, std::equal_to<>(), take_last(), "equal_to, take last");
        make_input(gen, n, true, k, v);
        run_in_place(pol, t, k, v, quarter_equal(), std::plus<double>(), "k / 4, plus");
        run_in_place(pol, t, k, v, quarter_equal(), take_first(), "k / 4, take first");
        run_in_place(pol, t, k, v, quarter_equal(), [] HPX_HOST_DEVICE(double, double b) { return b; },
                     "k / 4, take last (lambda)");
    }
}

// defaults (std::equal_to, std::plus), separate outputs; n == 0 -> +0, n == 1 -> +1
void test_defaults_and_ends(hip::target const& t) {
    std::vector<int32_t> k = {5, 5, 7, 7, 7, 5, 9};
    std::vector<int32_t> v = {1, 2, 3, 4, 5, 6, 7};
    auto dk = to_dev(k, t), dv = to_dev(v, t);
    dvec<int32_t> ok(k.size(), hip::allocator<int32_t>(t)), ov(k.size(), hip::allocator<int32_t>(t));
    auto r = hpx::parallel::reduce_by_key(ex::par, dk.begin(), dk.end(), dv.begin(), ok.begin(), ov.begin());
    HPX_TEST_EQ(r.first - ok.begin(), 4);
    HPX_TEST_EQ(r.second - ov.begin(), 4);
    expect_prefix(to_host(ok), std::vector<int32_t>{5, 7, 5, 9}, "defaults keys", k.size());
    expect_prefix(to_host(ov), std::vector<int32_t>{3, 12, 6, 7}, "defaults values", k.size());
    auto r0 = hpx::parallel::reduce_by_key(ex::par, dk.begin(), dk.begin(), dv.begin(), ok.begin(), ov.begin());
    HPX_TEST(r0.first == ok.begin() && r0.second == ov.begin());
    auto r1 = hpx::parallel::reduce_by_key(ex::seq, dk.begin() + 2, dk.begin() + 3, dv.begin() + 2, ok.begin(),
                                           ov.begin());
    HPX_TEST(r1.first == ok.begin() + 1 && r1.second == ov.begin() + 1);
    HPX_TEST_EQ(to_host(ok)[0], 7);
    HPX_TEST_EQ(to_host(ov)[0], 3);
    // the closure path at n == 0 and n == 1
    auto last = [] HPX_HOST_DEVICE(int32_t, int32_t b) { return b; };
    auto c0 = hpx::parallel::reduce_by_key(ex::par, dk.begin(), dk.begin(), dv.begin(), ok.begin(), ov.begin(),
                                           std::equal_to<>(), last);
    HPX_TEST(c0.first == ok.begin() && c0.second == ov.begin());
    auto c1 = hpx::parallel::reduce_by_key(ex::par, dk.begin() + 6, dk.end(), dv.begin() + 6, ok.begin(), ov.begin(),
                                           std::equal_to<>(), last);
    HPX_TEST(c1.first == ok.begin() + 1 && c1.second == ov.begin() + 1);
    HPX_TEST_EQ(to_host(ok)[0], 9);
    HPX_TEST_EQ(to_host(ov)[0], 7);
}

int hpx_main(int argc, char* argv[]) {
    unsigned seed = argc > 1 ? unsigned(std::strtoul(argv[1], nullptr, 10)) : std::random_device{}();
    std::cout << "using seed: " << seed << std::endl;
    std::mt19937_64 gen(seed);
    hip::target t;
    test_policy(ex::seq, t, gen);
    test_policy(ex::par, t, gen);
    test_policy(ex::par(ex::task), t, gen);
    test_defaults_and_ends(t);
    return hpx::finalize();
}

int main(int argc, char* argv[]) {
    HPX_TEST_EQ(hpx::init(argc, argv), 0);
    int errors = hpx::util::report_errors();
    if (!errors) std::cout << "reduce_by_key: all tests passed" << std::endl;
    return errors;
}
