// hpx::parallel::set_union, set_intersection, set_difference,
// set_symmetric_difference and includes (set_union.hpp:47 and its siblings,
// includes.hpp:129) through the HPX C++ layer, compiled by hipcc, under seq,
// par and par(task), on whole vectors and on the sub-range
// [begin() + 1, end()), against std::set_* / std::includes on the host.
//
//   std::less<int>, std::less<>, std::greater<>   the library's own kernels
//   [] (a, b) { (a >> 8) < (b >> 8) }             device closure: the low byte
//       of every element tags its source range and its index there, so the
//       comparison with the host's output shows that intersection and union
//       take tied elements from range 1 and that the ranks are counted right
#include <hpx/hpx.hpp>
#include <hpx/hpx_init.hpp>
#include <hpx/include/parallel_set_operations.hpp>
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

constexpr int kCanary = 0x5a5a5a5a;

// sorted multiset of n keys from [0, span), as key << 8 | tag with tag =
// range << 7 | (index & 127)
std::vector<int> tagged(std::mt19937& gen, std::size_t n, int span, int range) {
    std::vector<int> k(n);
    std::uniform_int_distribution<int> dist(0, span - 1);
    for (auto& x : k) x = dist(gen);
    std::sort(k.begin(), k.end());
    for (std::size_t i = 0; i < n; ++i) k[i] = (k[i] << 8) | (range << 7) | static_cast<int>(i & 127);
    return k;
}

template <typename Policy, typename Comp>
void run(Policy const& pol, hip::target const& t, std::vector<int> const& a, std::vector<int> const& b,
         std::size_t off, Comp comp, char const* what) {
    constexpr bool task = std::decay_t<Policy>::is_task;
    auto da = to_dev(a, t), db = to_dev(b, t);
    auto a0 = a.begin() + off, b0 = b.begin() + off;
    std::vector<int> exp[4];
    std::set_union(a0, a.end(), b0, b.end(), std::back_inserter(exp[0]), comp);
    std::set_intersection(a0, a.end(), b0, b.end(), std::back_inserter(exp[1]), comp);
    std::set_difference(a0, a.end(), b0, b.end(), std::back_inserter(exp[2]), comp);
    std::set_symmetric_difference(a0, a.end(), b0, b.end(), std::back_inserter(exp[3]), comp);
    for (int op = 0; op < 4; ++op) {
        auto o = to_dev(std::vector<int>(a.size() + b.size() + 2, kCanary), t);
        It f1 = da.begin() + off, l1 = da.end(), f2 = db.begin() + off, l2 = db.end(), d = o.begin() + 1;
        auto r = op == 0   ? hpx::parallel::set_union(pol, f1, l1, f2, l2, d, comp)
                 : op == 1 ? hpx::parallel::set_intersection(pol, f1, l1, f2, l2, d, comp)
                 : op == 2 ? hpx::set_difference(pol, f1, l1, f2, l2, d, comp)
                           : hpx::set_symmetric_difference(pol, f1, l1, f2, l2, d, comp);
        static_assert(std::is_same<decltype(r), std::conditional_t<task, hpx::future<It>, It>>::value,
                      "set operations return the output iterator (FwdIter3)");
        It end = value_of(std::move(r));
        HPX_TEST_EQ(static_cast<std::size_t>(end - d), exp[op].size());
        std::vector<int> want(a.size() + b.size() + 2, kCanary);
        std::copy(exp[op].begin(), exp[op].end(), want.begin() + 1);
        if (to_host(o) != want) {
            std::cout << what << ": op " << op << " differs from std::set_*" << std::endl;
            HPX_TEST(false);
        }
    }
    HPX_TEST(to_host(da) == a && to_host(db) == b);
    // includes: against std::includes both ways, and of the outputs
    auto inc = hpx::parallel::includes(pol, da.begin() + off, da.end(), db.begin() + off, db.end(), comp);
    static_assert(std::is_same<decltype(inc), std::conditional_t<task, hpx::future<bool>, bool>>::value,
                  "includes returns bool");
    HPX_TEST_EQ(value_of(std::move(inc)), std::includes(a0, a.end(), b0, b.end(), comp));
    HPX_TEST_EQ(value_of(hpx::includes(pol, db.begin() + off, db.end(), da.begin() + off, da.end(), comp)),
                std::includes(b0, b.end(), a0, a.end(), comp));
    auto du = to_dev(exp[0], t), di = to_dev(exp[1], t);
    HPX_TEST(value_of(hpx::includes(pol, du.begin(), du.end(), da.begin() + off, da.end(), comp)));
    HPX_TEST(value_of(hpx::includes(pol, du.begin(), du.end(), db.begin() + off, db.end(), comp)));
    HPX_TEST(value_of(hpx::includes(pol, da.begin() + off, da.end(), di.begin(), di.end(), comp)));
    HPX_TEST(value_of(hpx::includes(pol, da.begin() + off, da.end(), da.end(), da.end(), comp)));  // empty range 2
}

template <typename Policy>
void test_policy(Policy const& pol, hip::target const& t, std::mt19937& gen) {
    // 10007 + 9001 keys over 3 merge tiles of 2048, runs of about 5 per key
    // (and of about 1200: runs longer than half a tile)
    for (int span : {2000, 8}) {
        auto a = tagged(gen, 10007, span, 0), b = tagged(gen, 9001, span, 1);
        auto by_key = [] HPX_HOST_DEVICE(int x, int y) { return (x >> 8) < (y >> 8); };
        for (std::size_t off : {std::size_t(0), std::size_t(1)}) run(pol, t, a, b, off, by_key, "closure key >> 8");
        // the library's kernels: plain ints (the tags make every element distinct,
        // so strip them), ascending and descending
        std::vector<int> ka(a.size()), kb(b.size());
        std::transform(a.begin(), a.end(), ka.begin(), [](int x) { return x >> 8; });
        std::transform(b.begin(), b.end(), kb.begin(), [](int x) { return x >> 8; });
        for (std::size_t off : {std::size_t(0), std::size_t(1)}) {
            run(pol, t, ka, kb, off, std::less<int>(), "std::less<int>");
            run(pol, t, ka, kb, off, std::less<>(), "std::less<>");
        }
        std::reverse(ka.begin(), ka.end());
        std::reverse(kb.begin(), kb.end());
        run(pol, t, ka, kb, 1, std::greater<>(), "std::greater<>");
    }
    // empty ranges: dest + 0, includes of an empty range
    dvec d = to_dev({1, 2, 3}, t), o = to_dev({9, 9, 9}, t);
    HPX_TEST(value_of(hpx::parallel::set_union(pol, d.begin(), d.begin(), d.end(), d.end(), o.begin())) == o.begin());
    HPX_TEST(value_of(hpx::parallel::set_union(pol, d.begin(), d.end(), d.end(), d.end(), o.begin())) == o.end());
    HPX_TEST(value_of(hpx::parallel::includes(pol, d.begin(), d.begin(), d.end(), d.end())));
    HPX_TEST(!value_of(hpx::parallel::includes(pol, d.begin(), d.begin(), d.begin(), d.end())));
    HPX_TEST(to_host(o) == (std::vector<int>{1, 2, 3}));
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
    if (!errors) std::cout << "set_operations: all tests passed" << std::endl;
    return errors;
}
