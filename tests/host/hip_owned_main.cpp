// Stand-alone check of ipc_amd/csrc/hip_owned.hpp (no GPU): the handle template over malloc'd memory with a counting
// release function, and the real DevBuf where no device answers.  Built with -fsanitize=address,undefined by
// tests/test_hip_owned_cpu.py: a double release, a leak or a use after release ends the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../ipc_amd/csrc/hip_owned.hpp"

static int g_released = 0;
static std::atomic<int> g_live{0};
static hipError_t counting_free(int* p)
{
    std::free(p);
    ++g_released;
    return hipSuccess;
}
using Buf = ipc::Owned<int, counting_free, g_live>;
struct AllocBuf : Buf {                                // alloc() as DevBuf has it, over malloc: Owned::acquire
    hipError_t alloc(int v, bool fails = false)
    {
        return acquire([&](int** p) {
            if (fails) return hipErrorOutOfMemory;
            *p = static_cast<int*>(std::malloc(sizeof(int)));
            **p = v;
            return hipSuccess;
        });
    }
};

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static int* fresh(int v = 0)
{
    int* p = static_cast<int*>(std::malloc(sizeof(int)));
    *p = v;
    return p;
}

// the ipc_create pattern: two acquisitions, the second may fail -- the early return releases the first
static int two_steps(bool second_fails)
{
    Buf a(fresh());
    if (second_fails) return -1;
    Buf b(fresh());
    return 0;
}

struct Holder {                                        // as ipc_engine::SpecState: handles inside a struct inside a vector
    Buf poses;
    int tag = 0;
};

int main(int argc, char** argv)
{
    {   // every acquire is released exactly once on scope exit
        Buf a(fresh()), b(fresh()), empty;
        CHECK(g_live == 2 && a && b && !empty && empty.get() == nullptr);
    }
    CHECK(g_released == 2 && g_live == 0);

    g_released = 0;
    CHECK(two_steps(true) == -1 && g_released == 1 && g_live == 0);
    CHECK(two_steps(false) == 0 && g_released == 3 && g_live == 0);

    g_released = 0;
    {   // move construction hands over; move assignment frees the old value first
        Buf a(fresh(1)), b(fresh(2));
        Buf c(std::move(a));
        CHECK(!a && *c == 1 && g_released == 0 && g_live == 2);
        b = std::move(c);
        CHECK(g_released == 1 && g_live == 1 && !c && *b == 1);
        Buf& self = b;                                 // self-move is safe
        b = std::move(self);
        CHECK(g_released == 1 && g_live == 1 && b && *b == 1);
        b.reset();
        CHECK(g_released == 2 && g_live == 0 && !b);
        b.reset();                                     // (an empty handle releases nothing)
        CHECK(g_released == 2);
    }
    CHECK(g_released == 2 && g_live == 0);

    g_released = 0;
    {   // alloc() frees what the handle holds, then allocates; a failed one leaves the handle empty
        AllocBuf a;
        CHECK(a.alloc(1) == hipSuccess && *a == 1 && g_released == 0 && g_live == 1);
        CHECK(a.alloc(2) == hipSuccess && *a == 2 && g_released == 1 && g_live == 1);
        CHECK(a.alloc(3, true) != hipSuccess && !a && g_released == 2 && g_live == 0);
        CHECK(a.alloc(4) == hipSuccess && *a == 4 && g_released == 2 && g_live == 1);
    }
    CHECK(g_released == 3 && g_live == 0);

    g_released = 0;
    int* raw = nullptr;
    {   // release() gives the pointer up: the handle no longer frees (what ipc_engine::retired takes over)
        Buf a(fresh(7));
        raw = a.release();
        CHECK(!a && g_live == 0);
    }
    CHECK(g_released == 0 && *raw == 7);
    {
        std::vector<Buf> retired;
        retired.emplace_back(raw);
        CHECK(g_live == 1);
    }
    CHECK(g_released == 1 && g_live == 0);

    g_released = 0;
    {   // a vector of structs holding handles survives reallocation
        std::vector<Holder> v;
        for (int k = 0; k < 100; ++k) {
            v.emplace_back();
            v.back().poses.reset(fresh(k));
            v.back().tag = k;
        }
        CHECK(g_released == 0 && g_live == 100);
        bool same = true;
        for (int k = 0; k < 100; ++k) same = same && v[k].tag == k && *v[k].poses == k;
        CHECK(same);
    }
    CHECK(g_released == 100 && g_live == 0);

    if (argc > 1 && !std::strcmp(argv[1], "--no-device")) {
        // the real DevBuf / PinnedBuf / Event on a machine without a GPU: the HIP error comes back, the handle stays empty
        // (only there: a HIP runtime that finds a device keeps allocations of its own to the end of the process)
        ipc::DevBuf<double> d;
        CHECK(d.alloc(16) != hipSuccess && !d && d.get() == nullptr);
        ipc::PinnedBuf<int> p;
        CHECK(p.alloc(16) != hipSuccess && !p);
        ipc::Event e;
        CHECK(e.create(hipEventDisableTiming) != hipSuccess && !e);
    }
    CHECK(ipc::g_live_devbufs == 0 && ipc::g_live_pinned == 0 && ipc::g_live_events == 0);
    if (g_failed) return 1;
    std::printf("hip_owned OK\n");
    return 0;
}
