// ScratchCap of ipc_amd/csrc/hip_owned.hpp on the host alone: a group of three fake buffers, sized by different functions of
// the need, that count their live allocations and every alloc() call; the k-th call can be told to fail.  Needs the ROCm
// headers for hipError_t only; nothing of the runtime is linked.
#include "../../ipc_amd/csrc/hip_owned.hpp"

#include <cstdio>
#include <cstdlib>

static int g_live = 0, g_calls = 0, g_fail_at = 0;     // live allocations / alloc() calls so far / the call that fails (0: none)

struct FakeBuf {
    int* p = nullptr;
    size_t count = 0;
    ~FakeBuf() { reset(); }
    void reset()
    {
        if (p) { free(p); --g_live; }
        p = nullptr; count = 0;
    }
    hipError_t alloc(size_t n)
    {
        ++g_calls;
        reset();
        if (g_calls == g_fail_at) return hipErrorOutOfMemory;
        p = (int*)malloc(sizeof(int) * n); count = n; ++g_live;
        return hipSuccess;
    }
    int* get() const { return p; }
};

static int g_failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_failures; } } while (0)

struct Group {
    FakeBuf a, b, c;
    ipc::ScratchCap cap;
    hipError_t grow(size_t need) { return cap.grow(need, ipc::sized(a, need), ipc::sized(b, need + 1), ipc::sized(c, 3 * need)); }
};

int main()
{
    using namespace ipc;
    {
        Group g;
        CHECK(g.cap.size() == 0);
        CHECK(g.grow(10) == hipSuccess);
        CHECK(g.cap.size() == 10 && g_live == 3 && g_calls == 3);
        CHECK(g.a.count == 10 && g.b.count == 11 && g.c.count == 30);
        // (a) within the capacity: no allocation call, nothing moves
        int* a0 = g.a.p;
        CHECK(g.grow(10) == hipSuccess && g.grow(4) == hipSuccess && g.grow(0) == hipSuccess);
        CHECK(g_calls == 3 && g_live == 3 && g.a.p == a0 && g.cap.size() == 10);
        // (d) views are cut at the capacity: not at the need of the call (4) ...
        CHECK(g.cap.part(g.c, 0) == g.c.p && g.cap.part(g.c, 1) == g.c.p + 10 && g.cap.part(g.c, 2) == g.c.p + 20);
        // (b) a growth allocates every member anew; the capacity is the need
        const int before = g_calls;
        CHECK(g.grow(25) == hipSuccess);
        CHECK(g_calls == before + 3 && g_live == 3 && g.cap.size() == 25);
        CHECK(g.a.count == 25 && g.b.count == 26 && g.c.count == 75);
        // ... and not at the old capacity (10)
        CHECK(g.cap.part(g.c, 1) == g.c.p + 25 && g.cap.part(g.c, 2) == g.c.p + 50);
    }
    CHECK(g_live == 0);
    // (b) the first alloc() of a growth sees no live member: a probe in front of the three records the count at its turn
    {
        Group g;
        CHECK(g.grow(5) == hipSuccess && g_live == 3);
        struct Probe {
            int live_at_alloc = -1;
            void reset() {}
            hipError_t alloc(size_t) { live_at_alloc = g_live; return hipSuccess; }
        } probe;
        ScratchCap& cap = g.cap;
        CHECK(cap.grow(9, sized(probe, 0), sized(g.a, 9), sized(g.b, 10), sized(g.c, 27)) == hipSuccess);
        CHECK(probe.live_at_alloc == 0);               // every old array was gone before the first member was allocated
        CHECK(g_live == 3 && cap.size() == 9);
    }
    CHECK(g_live == 0);
    // (c) a failure at the k-th member: the error comes back, the capacity reads 0, and the next growth leaves one live
    // allocation per member -- nothing leaked, nothing released twice
    for (int k = 1; k <= 3; ++k) {
        Group g;
        CHECK(g.grow(8) == hipSuccess && g.cap.size() == 8);
        g_fail_at = g_calls + k;
        CHECK(g.grow(16) == hipErrorOutOfMemory);
        g_fail_at = 0;
        CHECK(g.cap.size() == 0);
        CHECK(g_live == k - 1);                        // the members before the one that failed
        CHECK(g.grow(1) == hipSuccess);                // (any need exceeds capacity 0)
        CHECK(g.cap.size() == 1 && g_live == 3);
        CHECK(g.a.count == 1 && g.b.count == 2 && g.c.count == 3);
        CHECK(g.cap.part(g.c, 2) == g.c.p + 2);
    }
    CHECK(g_live == 0);
    // a second capacity, in another unit, rides as the last member of the group: 0 with the first until everything is there
    {
        FakeBuf m, v;
        ScratchCap mat, vec;
        CHECK(mat.regrow(64, sized(m, 64), sized(v, 8), sized(vec, 8)) == hipSuccess && mat.size() == 64 && vec.size() == 8);
        g_fail_at = g_calls + 2;
        CHECK(mat.regrow(128, sized(m, 128), sized(v, 16), sized(vec, 16)) == hipErrorOutOfMemory);
        g_fail_at = 0;
        CHECK(mat.size() == 0 && vec.size() == 0 && g_live == 1);
        CHECK(mat.regrow(32, sized(m, 32), sized(v, 4), sized(vec, 4)) == hipSuccess && mat.size() == 32 && vec.size() == 4 && g_live == 2);
    }
    CHECK(g_live == 0);
    if (g_failures) return 1;
    printf("scratch_group OK\n");
    return 0;
}
