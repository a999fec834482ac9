// hpx::parallel::reverse, reverse_copy, rotate, rotate_copy, swap_ranges,
// replace, replace_if, replace_copy, replace_copy_if and adjacent_difference
// (reverse.hpp, rotate.hpp, swap_ranges.hpp, replace.hpp,
// adjacent_difference.hpp) through the HPX C++ layer, compiled by hipcc, under
// seq, par and par(task), on whole vectors and on the sub-range
// [begin() + 1, end()), against the std:: algorithms on the host.
//
//   functional::less_than<int>, std::minus<>      the library's own kernels
//   [] (x) { (x & 7) == 3 }, [] (x, y) { x ^ y }  device closures
#include <hpx/hpx.hpp>
#include <hpx/hpx_init.hpp>
#include <hpx/include/parallel_adjacent_difference.hpp>
#include <hpx/include/parallel_replace.hpp>
#include <hpx/include/parallel_reverse.hpp>
#include <hpx/include/parallel_rotate.hpp>
#include <hpx/include/parallel_swap_ranges.hpp>
#include <hpx/util/lightweight_test.hpp>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <iostream>
#include <numeric>
#include <random>
#include <type_traits>
#include <vector>

namespace hip = hpx::compute::hip;
namespace ex = hpx::parallel::execution;
namespace fn = hpx::compute::hip::functional;
using dvec = hpx::compute::vector<int, hip::allocator<int>>;
using It = dvec::iterator;
using hpx::parallel::util::tagged_pair;

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

constexpr int kCanary = 0x5a5a5a5a;

template <typename Policy>
void run(Policy const& pol, hip::target const& t, std::vector<int> const& a, std::size_t off) {
    constexpr bool task = std::decay_t<Policy>::is_task;
    const std::size_t n = a.size() - off;
    // a destination with a canary on both sides of [1, 1 + n)
    auto fresh = [&] { return to_dev(std::vector<int>(n + 2, kCanary), t); };
    auto framed = [&](std::vector<int> const& body) {
        std::vector<int> w(n + 2, kCanary);
        std::copy(body.begin(), body.end(), w.begin() + 1);
        return w;
    };
    std::vector<int> const sub(a.begin() + off, a.end());

    {  // reverse, reverse_copy
        auto d = to_dev(a, t);
        auto r = hpx::parallel::reverse(pol, d.begin() + off, d.end());
        static_assert(std::is_same<decltype(r), std::conditional_t<task, hpx::future<It>, It>>::value,
                      "reverse returns last");
        HPX_TEST(value_of(std::move(r)) == d.end());
        std::vector<int> want = a;
        std::reverse(want.begin() + off, want.end());
        HPX_TEST(to_host(d) == want);

        auto src = to_dev(a, t);
        auto o = fresh();
        auto rc = hpx::reverse_copy(pol, src.begin() + off, src.end(), o.begin() + 1);
        static_assert(std::is_same<decltype(rc), std::conditional_t<task, hpx::future<tagged_pair<It, It>>,
                                                                    tagged_pair<It, It>>>::value,
                      "reverse_copy returns tagged_pair<in, out>");
        auto pr = value_of(std::move(rc));
        HPX_TEST(pr.in() == src.end() && pr.out() == o.begin() + 1 + n);
        HPX_TEST(to_host(o) == framed(std::vector<int>(sub.rbegin(), sub.rend())));
        HPX_TEST(to_host(src) == a);
    }
    for (std::size_t mid : {std::size_t(0), std::size_t(1), n / 3, n - 1, n}) {  // rotate, rotate_copy
        if (mid > n) continue;
        auto d = to_dev(a, t);
        It first = d.begin() + off, nf = first + mid, last = d.end();
        auto r = hpx::parallel::rotate(pol, first, nf, last);
        static_assert(std::is_same<decltype(r), std::conditional_t<task, hpx::future<tagged_pair<It, It>>,
                                                                   tagged_pair<It, It>>>::value,
                      "rotate returns tagged_pair<begin, end>");
        auto pr = value_of(std::move(r));
        // (first + (last - new_first), last), checked on the plain members too
        HPX_TEST(pr.begin() == first + (last - nf) && pr.end() == last);
        HPX_TEST(pr.first == first + (n - mid) && pr.second == last);
        std::vector<int> want = a;
        std::rotate(want.begin() + off, want.begin() + off + mid, want.end());
        HPX_TEST(to_host(d) == want);

        auto src = to_dev(a, t);
        auto o = fresh();
        auto pc = value_of(hpx::rotate_copy(pol, src.begin() + off, src.begin() + off + mid, src.end(), o.begin() + 1));
        HPX_TEST(pc.in() == src.end() && pc.out() == o.begin() + 1 + n);
        HPX_TEST(to_host(o) == framed(std::vector<int>(want.begin() + off, want.end())));
        HPX_TEST(to_host(src) == a);
    }
    {  // swap_ranges: equal and different offsets inside 16 bytes
        for (std::size_t off2 : {off, off + 1}) {
            std::vector<int> b(a.size() + 1);
            std::iota(b.begin(), b.end(), 1000000);
            auto da = to_dev(a, t), db = to_dev(b, t);
            auto r = hpx::parallel::swap_ranges(pol, da.begin() + off, da.end(), db.begin() + off2);
            static_assert(std::is_same<decltype(r), std::conditional_t<task, hpx::future<It>, It>>::value,
                          "swap_ranges returns first2 + n");
            HPX_TEST(value_of(std::move(r)) == db.begin() + off2 + n);
            std::vector<int> wa = a, wb = b;
            std::swap_ranges(wa.begin() + off, wa.end(), wb.begin() + off2);
            HPX_TEST(to_host(da) == wa && to_host(db) == wb);
        }
    }
    {  // replace family: mapped predicates and a device closure
        auto d = to_dev(a, t);
        HPX_TEST(value_of(hpx::parallel::replace(pol, d.begin() + off, d.end(), 7, -7)) == d.end());
        std::vector<int> want = a;
        std::replace(want.begin() + off, want.end(), 7, -7);
        HPX_TEST(to_host(d) == want);

        d = to_dev(a, t);
        auto r = hpx::parallel::replace_if(pol, d.begin() + off, d.end(), fn::less_than<int>{20}, 99);
        static_assert(std::is_same<decltype(r), std::conditional_t<task, hpx::future<It>, It>>::value,
                      "replace_if returns last");
        HPX_TEST(value_of(std::move(r)) == d.end());
        want = a;
        std::replace_if(want.begin() + off, want.end(), [](int x) { return x < 20; }, 99);
        HPX_TEST(to_host(d) == want);

        d = to_dev(a, t);
        auto low3 = [] HPX_HOST_DEVICE(int x) { return (x & 7) == 3; };
        HPX_TEST(value_of(hpx::replace_if(pol, d.begin() + off, d.end(), low3, -1)) == d.end());
        want = a;
        std::replace_if(want.begin() + off, want.end(), low3, -1);
        HPX_TEST(to_host(d) == want);

        auto src = to_dev(a, t);
        auto o = fresh();
        auto pc = value_of(hpx::parallel::replace_copy(pol, src.begin() + off, src.end(), o.begin() + 1, 7, -7));
        HPX_TEST(pc.in() == src.end() && pc.out() == o.begin() + 1 + n);
        std::vector<int> body(n);
        std::replace_copy(sub.begin(), sub.end(), body.begin(), 7, -7);
        HPX_TEST(to_host(o) == framed(body));

        o = fresh();
        auto pi = value_of(hpx::parallel::replace_copy_if(pol, src.begin() + off, src.end(), o.begin() + 1, low3, -1));
        HPX_TEST(pi.in() == src.end() && pi.out() == o.begin() + 1 + n);
        std::replace_copy_if(sub.begin(), sub.end(), body.begin(), low3, -1);
        HPX_TEST(to_host(o) == framed(body));
        HPX_TEST(to_host(src) == a);
    }
    {  // adjacent_difference: std::minus (default), and a device closure
        auto src = to_dev(a, t);
        auto o = fresh();
        auto r = hpx::parallel::adjacent_difference(pol, src.begin() + off, src.end(), o.begin() + 1);
        static_assert(std::is_same<decltype(r), std::conditional_t<task, hpx::future<It>, It>>::value,
                      "adjacent_difference returns dest + n");
        HPX_TEST(value_of(std::move(r)) == o.begin() + 1 + n);
        std::vector<int> body(n);
        std::adjacent_difference(sub.begin(), sub.end(), body.begin());
        HPX_TEST(to_host(o) == framed(body));

        o = fresh();
        auto x_or = [] HPX_HOST_DEVICE(int x, int y) { return x ^ y; };
        HPX_TEST(value_of(hpx::adjacent_difference(pol, src.begin() + off, src.end(), o.begin() + 1, x_or)) ==
                 o.begin() + 1 + n);
        std::adjacent_difference(sub.begin(), sub.end(), body.begin(), x_or);
        HPX_TEST(to_host(o) == framed(body));
        HPX_TEST(to_host(src) == a);
    }
}

template <typename Policy>
void test_policy(Policy const& pol, hip::target const& t, std::mt19937& gen) {
    // 5003 elements: past the 4-KiB threshold of the shifted-load path
    for (std::size_t n : {std::size_t(5003), std::size_t(37)}) {
        std::vector<int> a(n);
        std::uniform_int_distribution<int> dist(0, 40);
        for (auto& x : a) x = dist(gen);
        for (std::size_t off : {std::size_t(0), std::size_t(1)}) run(pol, t, a, off);
    }
    // empty ranges
    dvec d = to_dev({1, 2, 3}, t), o = to_dev({9, 9, 9}, t);
    HPX_TEST(value_of(hpx::parallel::reverse(pol, d.begin(), d.begin())) == d.begin());
    HPX_TEST(value_of(hpx::parallel::reverse_copy(pol, d.begin(), d.begin(), o.begin())).out() == o.begin());
    HPX_TEST(value_of(hpx::parallel::adjacent_difference(pol, d.begin(), d.begin(), o.begin())) == o.begin());
    HPX_TEST(to_host(d) == (std::vector<int>{1, 2, 3}) && to_host(o) == (std::vector<int>{9, 9, 9}));
    // overlapping ranges are refused with mapped functors and with device
    // closures alike (an exception_list; in a future under a task policy)
    auto refused = [&](auto call) {
        try {
            value_of(call());
        } catch (hpx::exception_list const&) {
            return true;
        }
        return false;
    };
    auto odd = [] HPX_HOST_DEVICE(int x) { return (x & 1) != 0; };
    auto x_or = [] HPX_HOST_DEVICE(int x, int y) { return x ^ y; };
    HPX_TEST(refused([&] { return hpx::parallel::adjacent_difference(pol, d.begin(), d.end(), d.begin()); }));
    HPX_TEST(refused([&] { return hpx::parallel::adjacent_difference(pol, d.begin(), d.end(), d.begin(), x_or); }));
    HPX_TEST(refused([&] { return hpx::parallel::adjacent_difference(pol, d.begin(), d.end() - 1, d.begin() + 1, x_or); }));
    HPX_TEST(refused([&] {
        return hpx::parallel::replace_copy_if(pol, d.begin(), d.end() - 1, d.begin() + 1, fn::less_than<int>{2}, 0);
    }));
    HPX_TEST(refused([&] { return hpx::parallel::replace_copy_if(pol, d.begin(), d.end() - 1, d.begin() + 1, odd, 0); }));
    HPX_TEST(to_host(d) == (std::vector<int>{1, 2, 3}));
}

int hpx_main(int, char*[]) {
    std::mt19937 gen(20261021);
    hip::target t;
    test_policy(ex::seq, t, gen);
    test_policy(ex::par, t, gen);
    test_policy(ex::par(ex::task), t, gen);
    return hpx::finalize();
}

int main(int argc, char* argv[]) {
    HPX_TEST_EQ(hpx::init(argc, argv), 0);
    int errors = hpx::util::report_errors();
    if (!errors) std::cout << "permute: all tests passed" << std::endl;
    return errors;
}
