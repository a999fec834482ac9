// hpx::parallel::unique_copy and unique (unique.hpp:311,612) through the HPX
// C++ layer, compiled by hipcc, under seq, par and par(task), out of place
// and in place, on the whole vector and on the sub-range [begin() + 1, end()),
// against std::unique_copy / std::unique on the host.  The known-answer shape
// of the reference's tests: 10007 ints drawn from 7 neighbouring values.
//
//   std::equal_to<int>, std::equal_to<>    the library's own kernels
//   fn::equal_shifted<int>{2}              the library's own kernels
//   [v] (a, b) { a == b && b == v }        device closure (a relation that
//                                          implies value equality)
//   std::equal_to<> under x -> x / 4       device closure with a projection
#include <hpx/hpx.hpp>
#include <hpx/hpx_init.hpp>
#include <hpx/include/parallel_unique.hpp>
#include <hpx/util/lightweight_test.hpp>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <iostream>
#include <iterator>
#include <random>
#include <type_traits>
#include <vector>

namespace hip = hpx::compute::hip;
namespace ex = hpx::parallel::execution;
namespace fn = hpx::compute::hip::functional;
using dvec = hpx::compute::vector<int, hip::allocator<int>>;
using It = dvec::iterator;

std::vector<int> to_host(dvec const& d) {
    std::vector<int> h(d.size());
    hpx::parallel::copy(ex::par, d.begin(), d.end(), h.begin());
    return h;
}
dvec to_dev(std::vector<int> const& h, hip::target const& t) {
    dvec d(h.size(), hip::allocator<int>(t));
    hpx::parallel::copy(ex::par, h.begin(), h.end(), d.begin());
    return d;
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

constexpr int kCanary = 0x5a5a5a5a;

bool same(std::vector<int> const& got, std::size_t at, std::vector<int> const& exp, char const* what) {
    for (std::size_t i = 0; i < exp.size(); ++i)
        if (got[at + i] != exp[i]) {
            std::cout << what << ": first mismatch at " << i << std::endl;
            HPX_TEST(false);
            return false;
        }
    return true;
}

// call(first, last, dest) -> unique_copy's result, call_in_place(first, last)
// -> unique's; host_rel: the relation on the host.
template <typename Policy, typename Copy, typename InPlace, typename HostRel>
void run(Policy const&, hip::target const& t, std::vector<int> const& a, std::size_t off, Copy call,
         InPlace call_in_place, HostRel host_rel, char const* what) {
    constexpr bool task = std::decay_t<Policy>::is_task;
    using pair2 = hpx::parallel::util::tagged_pair<It, It>;
    std::vector<int> exp;
    std::unique_copy(a.begin() + off, a.end(), std::back_inserter(exp), host_rel);
    {  // unique_copy
        auto d = to_dev(a, t);
        auto o = to_dev(std::vector<int>(a.size() + 2, kCanary), t);
        auto c = call(d.begin() + off, d.end(), o.begin() + 1);
        static_assert(std::is_same<decltype(c), std::conditional_t<task, hpx::future<pair2>, pair2>>::value,
                      "unique_copy result type");
        pair2 r = value_of(std::move(c));
        HPX_TEST(r.in() == d.end());
        HPX_TEST_EQ(std::size_t(r.out() - (o.begin() + 1)), exp.size());
        auto ho = to_host(o);
        same(ho, 1, exp, what);
        HPX_TEST(ho[0] == kCanary && ho[1 + exp.size()] == kCanary);
        same(to_host(d), 0, a, what);
    }
    {  // unique: std::unique gives the same new end and the same kept elements
        std::vector<int> b(a);
        auto e = std::unique(b.begin() + off, b.end(), host_rel);
        HPX_TEST_EQ(std::size_t(e - (b.begin() + off)), exp.size());
        auto d = to_dev(a, t);
        auto c = call_in_place(d.begin() + off, d.end());
        static_assert(std::is_same<decltype(c), std::conditional_t<task, hpx::future<It>, It>>::value,
                      "unique result type");
        It r = value_of(std::move(c));
        HPX_TEST_EQ(std::size_t(r - (d.begin() + off)), exp.size());
        auto hd = to_host(d);
        same(hd, off, exp, what);
        // in front of the range and from the new end onward: the old values
        same(hd, 0, std::vector<int>(a.begin(), a.begin() + off), what);
        same(hd, off + exp.size(), std::vector<int>(a.begin() + off + exp.size(), a.end()), what);
    }
}

template <typename Policy>
void test_policy(Policy const& pol, hip::target const& t, std::mt19937& gen) {
    std::vector<int> a(10007);
    const int base = static_cast<int>(gen() % 1000);
    for (auto& x : a) x = base + static_cast<int>(gen() % 7);
    const int v = base + 3;
    for (std::size_t off : {std::size_t(0), std::size_t(1)}) {
        run(pol, t, a, off,
            [&](It f, It l, It d) { return hpx::parallel::unique_copy(pol, f, l, d); },
            [&](It f, It l) { return hpx::parallel::unique(pol, f, l); }, std::equal_to<int>(), "default");
        run(pol, t, a, off,
            [&](It f, It l, It d) { return hpx::parallel::unique_copy(pol, f, l, d, std::equal_to<int>()); },
            [&](It f, It l) { return hpx::unique(pol, f, l, std::equal_to<>()); }, std::equal_to<int>(),
            "std::equal_to");
        auto rel = [v] HPX_HOST_DEVICE(int x, int y) { return x == y && y == v; };
        run(pol, t, a, off, [&](It f, It l, It d) { return hpx::parallel::unique_copy(pol, f, l, d, rel); },
            [&](It f, It l) { return hpx::parallel::unique(pol, f, l, rel); }, rel, "closure a == b && b == v");
        auto host_quarter = [](int x, int y) { return x / 4 == y / 4; };
        run(pol, t, a, off,
            [&](It f, It l, It d) { return hpx::unique_copy(pol, f, l, d, std::equal_to<>(), quarter{}); },
            [&](It f, It l) { return hpx::parallel::unique(pol, f, l, std::equal_to<>(), quarter{}); }, host_quarter,
            "projection x / 4");
        auto host_shift = [](int x, int y) { return (x >> 2) == (y >> 2); };
        run(pol, t, a, off,
            [&](It f, It l, It d) { return hpx::parallel::unique_copy(pol, f, l, d, fn::equal_shifted<int>{2}); },
            [&](It f, It l) { return hpx::parallel::unique(pol, f, l, fn::equal_shifted<int>{2}); }, host_shift,
            "equal_shifted");
    }
    // n == 0 and n == 1: first + count
    dvec d = to_dev({7, 7, 7, 7}, t), o = to_dev({1, 1, 1, 1}, t);
    auto r0 = value_of(hpx::parallel::unique_copy(pol, d.begin(), d.begin(), o.begin()));
    HPX_TEST(r0.in() == d.begin() && r0.out() == o.begin());
    auto r1 = value_of(hpx::parallel::unique_copy(pol, d.begin(), d.begin() + 1, o.begin()));
    HPX_TEST(r1.in() == d.begin() + 1 && r1.out() == o.begin() + 1);
    HPX_TEST(value_of(hpx::parallel::unique(pol, d.begin(), d.begin())) == d.begin());
    HPX_TEST(value_of(hpx::parallel::unique(pol, d.begin(), d.begin() + 1)) == d.begin() + 1);
    HPX_TEST(value_of(hpx::parallel::unique(pol, d.begin(), d.end())) == d.begin() + 1);
    HPX_TEST(to_host(o) == (std::vector<int>{7, 1, 1, 1}));
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
    if (!errors) std::cout << "unique: all tests passed" << std::endl;
    return errors;
}
