// hpx::parallel::partition_copy, stable_partition, partition, remove_copy_if,
// remove_copy, remove_if and remove (partition.hpp:292,1063,1350,
// remove_copy.hpp:173,350, remove.hpp:290,367) through the HPX C++ layer,
// compiled by hipcc, under par and par(task), out of place and in place,
// against a host loop:
//
//   functional::less_than<T>{50}           the library's own kernels
//   [] HPX_HOST_DEVICE (T x) { x % 3 == 0 } device closure
//   in_band{lo, hi}                        device closure, a functor with state
//
// at T-1, T+1 and 65T+3 elements (T = the kernel's tile, 128 KiB of elements).
#include <hpx/hpx.hpp>
#include <hpx/hpx_init.hpp>
#include <hpx/include/parallel_partition.hpp>
#include <hpx/include/parallel_remove.hpp>
#include <hpx/util/lightweight_test.hpp>

#include <cstdint>
#include <iostream>
#include <random>
#include <type_traits>
#include <vector>

namespace hip = hpx::compute::hip;
namespace ex = hpx::parallel::execution;
namespace fn = hpx::compute::hip::functional;
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

template <typename T>
struct in_band {
    T lo, hi;
    HPX_HOST_DEVICE bool operator()(T x) const { return lo <= x && x < hi; }
};

template <typename R>
R value_of(R r) {
    return r;
}
template <typename R>
R value_of(hpx::future<R> f) {
    return f.get();
}

template <typename T>
bool expect_range(std::vector<T> const& got, std::size_t at, std::vector<T> const& exp, char const* what,
                  std::size_t n) {
    for (std::size_t i = 0; i < exp.size(); ++i)
        if (!(got[at + i] == exp[i])) {
            std::cout << what << " n=" << n << ": first mismatch at " << i << std::endl;
            HPX_TEST(false);
            return false;
        }
    return true;
}

constexpr int64_t kCanary = 0x5a5a5a5a;

template <typename Policy, typename T, typename Pred>
void run_all(Policy const& pol, hip::target const& t, std::vector<T> const& a, Pred pred, char const* what) {
    constexpr bool task = std::decay_t<Policy>::is_task;
    using It = typename dvec<T>::iterator;
    const std::size_t n = a.size();
    std::vector<T> acc, rej, both;
    for (T x : a) (pred(x) ? acc : rej).push_back(x);
    both = acc;
    both.insert(both.end(), rej.begin(), rej.end());
    const std::vector<T> blank(n + 1, T(kCanary));

    {  // partition_copy, out of place
        auto d = to_dev(a, t);
        auto ot = to_dev(blank, t), of = to_dev(blank, t);
        auto call = hpx::parallel::partition_copy(pol, d.begin(), d.end(), ot.begin(), of.begin(), pred);
        static_assert(std::is_same<decltype(call), std::conditional_t<task, hpx::future<hpx::parallel::util::tagged_tuple<It, It, It>>,
                                                                      hpx::parallel::util::tagged_tuple<It, It, It>>>::value,
                      "partition_copy result type");
        auto r = value_of(std::move(call));
        HPX_TEST(r.in() == d.end());
        HPX_TEST_EQ(std::size_t(r.out1() - ot.begin()), acc.size());
        HPX_TEST_EQ(std::size_t(r.out2() - of.begin()), rej.size());
        auto ht = to_host(ot), hf = to_host(of);
        expect_range(ht, 0, acc, what, n);
        expect_range(hf, 0, rej, what, n);
        HPX_TEST(ht[acc.size()] == T(kCanary) && hf[rej.size()] == T(kCanary));
        expect_range(to_host(d), 0, a, what, n);
    }
    {  // partition_copy, the accepted side in place
        auto d = to_dev(a, t);
        auto of = to_dev(blank, t);
        auto r = value_of(hpx::parallel::partition_copy(pol, d.begin(), d.end(), d.begin(), of.begin(), pred));
        HPX_TEST_EQ(std::size_t(r.out1() - d.begin()), acc.size());
        HPX_TEST_EQ(std::size_t(r.out2() - of.begin()), rej.size());
        auto hd = to_host(d);
        expect_range(hd, 0, acc, what, n);
        // from the new end onward the old values
        expect_range(hd, acc.size(), std::vector<T>(a.begin() + acc.size(), a.end()), what, n);
        expect_range(to_host(of), 0, rej, what, n);
    }
    {  // stable_partition and partition
        auto d = to_dev(a, t);
        auto call = hpx::parallel::stable_partition(pol, d.begin(), d.end(), pred);
        static_assert(std::is_same<decltype(call), std::conditional_t<task, hpx::future<It>, It>>::value,
                      "stable_partition result type");
        It r = value_of(std::move(call));
        HPX_TEST_EQ(std::size_t(r - d.begin()), acc.size());
        expect_range(to_host(d), 0, both, what, n);
        auto d2 = to_dev(a, t);
        It r2 = value_of(hpx::partition(pol, d2.begin(), d2.end(), pred));
        HPX_TEST_EQ(std::size_t(r2 - d2.begin()), acc.size());
        expect_range(to_host(d2), 0, both, what, n);
    }
    {  // remove_copy_if out of place, remove_if in place
        auto d = to_dev(a, t);
        auto o = to_dev(blank, t);
        auto call = hpx::parallel::remove_copy_if(pol, d.begin(), d.end(), o.begin(), pred);
        static_assert(std::is_same<decltype(call), std::conditional_t<task, hpx::future<hpx::parallel::util::tagged_pair<It, It>>,
                                                                      hpx::parallel::util::tagged_pair<It, It>>>::value,
                      "remove_copy_if result type");
        auto r = value_of(std::move(call));
        HPX_TEST(r.in() == d.end());
        HPX_TEST_EQ(std::size_t(r.out() - o.begin()), rej.size());
        auto ho = to_host(o);
        expect_range(ho, 0, rej, what, n);
        HPX_TEST(ho[rej.size()] == T(kCanary));
        It e = value_of(hpx::parallel::remove_if(pol, d.begin(), d.end(), pred));
        HPX_TEST_EQ(std::size_t(e - d.begin()), rej.size());
        auto hd = to_host(d);
        expect_range(hd, 0, rej, what, n);
        expect_range(hd, rej.size(), std::vector<T>(a.begin() + rej.size(), a.end()), what, n);
    }
}

template <typename Policy, typename T>
void run_remove_value(Policy const& pol, hip::target const& t, std::vector<T> const& a, T value) {
    const std::size_t n = a.size();
    std::vector<T> kept;
    for (T x : a)
        if (!(x == value)) kept.push_back(x);
    auto d = to_dev(a, t);
    dvec<T> o(n + 1, hip::allocator<T>(t));
    auto r = value_of(hpx::remove_copy(pol, d.begin(), d.end(), o.begin(), value));
    HPX_TEST(r.in() == d.end());
    HPX_TEST_EQ(std::size_t(r.out() - o.begin()), kept.size());
    expect_range(to_host(o), 0, kept, "remove_copy", n);
    auto e = value_of(hpx::remove(pol, d.begin(), d.end(), value));
    HPX_TEST_EQ(std::size_t(e - d.begin()), kept.size());
    expect_range(to_host(d), 0, kept, "remove", n);
}

template <typename Policy, typename T>
void test_policy(Policy const& pol, hip::target const& t, std::mt19937_64& gen) {
    constexpr std::size_t tile = 131072 / sizeof(T);
    for (std::size_t n : {tile - 1, tile + 1, 65 * tile + 3}) {
        std::vector<T> a(n);
        for (auto& x : a) x = T(gen() % 100);
        run_all(pol, t, a, fn::less_than<T>{T(50)}, "less_than");
        run_all(pol, t, a, in_band<T>{T(20), T(70)}, "functor with state");
        if constexpr (std::is_integral<T>::value)
            run_all(pol, t, a, [] HPX_HOST_DEVICE(T x) { return x % 3 == 0; }, "lambda x % 3 == 0");
        else
            run_all(pol, t, a, [] HPX_HOST_DEVICE(T x) { return x * T(0.5) > T(30); }, "lambda x / 2 > 30");
        for (auto& x : a) x = T(gen() % 4);
        run_remove_value(pol, t, a, T(3));
    }
    // empty ranges: the un-advanced iterators
    dvec<T> d(4, hip::allocator<T>(t)), o(4, hip::allocator<T>(t));
    auto r = value_of(hpx::parallel::partition_copy(pol, d.begin(), d.begin(), o.begin(), o.begin() + 2,
                                                    [] HPX_HOST_DEVICE(T) { return true; }));
    HPX_TEST(r.in() == d.begin() && r.out1() == o.begin() && r.out2() == o.begin() + 2);
    HPX_TEST(value_of(hpx::parallel::stable_partition(pol, d.begin(), d.begin(), in_band<T>{T(0), T(1)})) == d.begin());
    HPX_TEST(value_of(hpx::parallel::remove(pol, d.begin(), d.begin(), T(1))) == d.begin());
}

int hpx_main(int, char*[]) {
    std::mt19937_64 gen(20261020);
    hip::target t;
    test_policy<decltype(ex::par), int64_t>(ex::par, t, gen);
    test_policy<decltype(ex::par(ex::task)), int64_t>(ex::par(ex::task), t, gen);
    test_policy<decltype(ex::par), int32_t>(ex::par, t, gen);
    test_policy<decltype(ex::par(ex::task)), double>(ex::par(ex::task), t, gen);
    return hpx::finalize();
}

int main(int argc, char* argv[]) {
    HPX_TEST_EQ(hpx::init(argc, argv), 0);
    int errors = hpx::util::report_errors();
    if (!errors) std::cout << "partition: all tests passed" << std::endl;
    return errors;
}
