// The owning buffer type of the context (cmc_fluid_solver_amd/csrc/fs3d_buf.h) on a CPU: malloc / free behind a policy that
// counts and can be told to fail.  Built with the address and undefined-behaviour sanitizers by tests/test_dev_buffer.py and
// run as its own program: `dev_buffer_test N` runs case N (1 .. 6), exit status 1 at the first violated statement; case 7 --
// nothing is live once a case has gone out of scope -- is checked after every case.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "../cmc_fluid_solver_amd/csrc/fs3d_buf.h"

struct TestMem {
    static long long live, total, frees;
    static int fail_in;                      // > 0: the fail_in-th allocation from now fails
    static void *alloc(size_t bytes)
    {
        if (fail_in > 0 && --fail_in == 0) return nullptr;
        void *p = malloc(bytes ? bytes : 1);
        if (p) { live++; total++; }
        return p;
    }
    static void free(void *p) { ::free(p); live--; frees++; }
};
long long TestMem::live = 0, TestMem::total = 0, TestMem::frees = 0;
int TestMem::fail_in = 0;

typedef OwnedBuf<TestMem, int> IntBuf;
typedef OwnedBuf<TestMem> VoidBuf;
static_assert(!std::is_copy_constructible<IntBuf>::value && !std::is_copy_assignable<IntBuf>::value, "a buffer is move-only");
static_assert(std::is_move_constructible<IntBuf>::value && std::is_move_assignable<IntBuf>::value, "a buffer is move-only");

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static bool empty(const RawBuf<TestMem> &b) { return b.raw() == nullptr && b.bytes() == 0 && !b.holds(0) && !b.holds(1); }

static void case_default_and_reset()
{
    IntBuf b;
    long long n = 0;
    CHECK(empty(b) && (int *)b == nullptr && !b);
    b.reset(&n); b.reset(&n); b.reset();
    CHECK(empty(b) && n == 0 && TestMem::total == 0 && TestMem::frees == 0);
    CHECK(b.reserve(40, &n) && n == 1);
    b.reset(&n);
    CHECK(empty(b) && n == 2 && TestMem::live == 0);
    b.reset(&n);                             // twice is harmless
    CHECK(empty(b) && n == 2 && TestMem::frees == 1);
}

static void case_reserve_grows_only()
{
    IntBuf b;
    long long n = 0;
    bool fresh = false;
    CHECK(b.reserve(64, &n, &fresh) && fresh && n == 1 && b.holds(64) && !b.holds(65) && b.bytes() == 64);
    int *const p = b;
    for (int i = 0; i < 16; i++) p[i] = i;   // the whole capacity is ours (the sanitizer watches)
    fresh = false;
    CHECK(b.reserve(64, &n, &fresh) && b.reserve(8, &n, &fresh) && !fresh && n == 1 && (int *)b == p && b.bytes() == 64);
    CHECK(TestMem::total == 1 && TestMem::frees == 0);
    CHECK(b.reserve(65, &n, &fresh) && fresh && n == 3 && b.holds(65) && b.bytes() == 65);
    CHECK(TestMem::total == 2 && TestMem::frees == 1 && TestMem::live == 1);
    CHECK(b.reserve(100) && TestMem::total == 3 && n == 3);      // no counter: nothing counted
}

static void case_replace_is_exact()
{
    VoidBuf b;
    long long n = 0;
    CHECK(b.replace(48, &n) && n == 1 && b.bytes() == 48);
    CHECK(b.replace(48, &n) && n == 3 && b.bytes() == 48);       // the upload's rule: the same size again is a new allocation
    CHECK(TestMem::total == 2 && TestMem::frees == 1 && TestMem::live == 1);
    CHECK(b.replace(16, &n) && n == 5 && b.bytes() == 16 && !b.holds(48));
    ((char *)b)[15] = 1;
}

static void case_failure_leaves_it_empty()
{
    IntBuf b;
    long long n = 0;
    TestMem::fail_in = 1;
    CHECK(!b.reserve(32, &n) && empty(b) && n == 0 && TestMem::live == 0);          // empty before
    CHECK(b.reserve(32, &n) && b.holds(32) && n == 1);
    TestMem::fail_in = 1;
    CHECK(!b.reserve(64, &n) && empty(b));                                          // held a smaller one
    CHECK(n == 2 && TestMem::frees == 1 && TestMem::live == 0);                     // ... freed exactly once
    CHECK(b.reserve(64, &n) && b.holds(64) && n == 3 && TestMem::live == 1);        // a later reserve succeeds
    TestMem::fail_in = 1;
    CHECK(!b.replace(8, &n) && empty(b) && n == 4 && TestMem::live == 0);
}

static void case_all_or_nothing()
{
    const size_t sz[4] = {24, 24, 16, 160};
    for (int k = 1; k <= 4; k++) {
        IntBuf a, b;
        VoidBuf c, d;
        long long n = 0;
        CHECK(c.reserve(8, &n));             // one of them holds a smaller buffer already
        TestMem::fail_in = k;
        CHECK(!reserve_all<TestMem>({{&a, sz[0]}, {&b, sz[1]}, {&c, sz[2]}, {&d, sz[3]}}, &n));
        CHECK(empty(a) && empty(b) && empty(c) && empty(d) && TestMem::live == 0);
        CHECK(n == TestMem::total + TestMem::frees && TestMem::total == TestMem::frees);
        TestMem::fail_in = 0; TestMem::total = 0; TestMem::frees = 0;
    }
    IntBuf a, b;
    VoidBuf c, d;
    long long n = 0;
    bool fresh = false;
    CHECK(reserve_all<TestMem>({{&a, sz[0]}, {&b, sz[1]}, {&c, sz[2]}, {&d, sz[3]}}, &n, &fresh));
    CHECK(fresh && n == 4 && TestMem::total == 4 && TestMem::live == 4);
    CHECK(a.holds(sz[0]) && b.holds(sz[1]) && c.holds(sz[2]) && d.holds(sz[3]));
    fresh = false;
    CHECK(reserve_all<TestMem>({{&a, sz[0]}, {&b, sz[1]}, {&c, sz[2]}, {&d, sz[3]}}, &n, &fresh));
    CHECK(!fresh && n == 4 && TestMem::total == 4 && TestMem::frees == 0);          // a second time allocates nothing
    // a larger group: the members that are too small are made again, the others stay
    CHECK(reserve_all<TestMem>({{&a, sz[0]}, {&b, 2 * sz[1]}}, &n, &fresh) && fresh && n == 6 && b.holds(2 * sz[1]));
}

static void case_moves()
{
    IntBuf a;
    CHECK(a.reserve(32));
    int *const p = a;
    IntBuf b(std::move(a));
    CHECK(empty(a) && (int *)b == p && b.bytes() == 32 && TestMem::total == 1 && TestMem::frees == 0);
    IntBuf c;
    c = std::move(b);
    CHECK(empty(b) && (int *)c == p && c.bytes() == 32 && TestMem::frees == 0);
    IntBuf d;
    CHECK(d.reserve(8) && TestMem::live == 2);
    d = std::move(c);                        // onto a non-empty buffer: its old memory is freed once
    CHECK(empty(c) && (int *)d == p && d.bytes() == 32 && TestMem::frees == 1 && TestMem::live == 1);
    IntBuf &self = d;
    d = std::move(self);
    CHECK((int *)d == p && d.bytes() == 32 && TestMem::frees == 1);
}

int main(int argc, char **argv)
{
    void (*const cases[])() = {case_default_and_reset, case_reserve_grows_only, case_replace_is_exact, case_failure_leaves_it_empty,
                               case_all_or_nothing, case_moves};
    const int n = (int)(sizeof cases / sizeof cases[0]), which = argc > 1 ? atoi(argv[1]) : 0;
    if (which < 1 || which > n) { fprintf(stderr, "usage: dev_buffer_test CASE (1 .. %d)\n", n); return 2; }
    cases[which - 1]();
    CHECK(TestMem::live == 0 && TestMem::total == TestMem::frees);      // the destructors have freed what the case left
    printf("case %d ok: %lld allocations, %lld frees\n", which, TestMem::total, TestMem::frees);
    return 0;
}
