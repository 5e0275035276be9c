/*
 * own_check.cpp -- the resource owners of csrc/lh_hip_own.h against the stand-in HIP of this directory: what a batch or a
 * handle relies on when it frees its resources by being deleted.  Stand-alone (tests/test_hip_owners.py builds and runs
 * it); exit status 0 = every check held, otherwise the failed checks are on stderr.
 */
#include "lh_hip_own.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

typedef std::vector < std::string > Log;

template < typename Buf > static void
check_buffer(void)
{
    /* a scope exit leaves nothing live; alloc in place of something held releases it first */
    {
        Buf     a;
        CHECK(a.get() == nullptr && a.cap() == 0);
        CHECK(a.alloc(10) == hipSuccess && a.get() != nullptr && a.cap() == 10);
        CHECK(stub::live.size() == 1);
        CHECK(a.alloc(20) == hipSuccess && a.cap() == 20 && stub::live.size() == 1);
        a.release();
        CHECK(a.get() == nullptr && a.cap() == 0 && stub::live.empty());
        a.release();            /* (nothing held: nothing happens) */
        CHECK(a.alloc(5) == hipSuccess);
    }
    CHECK(stub::live.empty());
    /* a moved-from owner releases nothing; a move onto an owner releases what it held */
    {
        Buf     a, c;
        CHECK(a.alloc(8) == hipSuccess && c.alloc(3) == hipSuccess);
        void   *const p = a.get();
        Buf     b(std::move(a));
        CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == p && b.cap() == 8 && stub::live.size() == 2);
        c = std::move(b);
        CHECK(b.get() == nullptr && c.get() == p && c.cap() == 8 && stub::live.size() == 1);
    }
    CHECK(stub::live.empty());
    /* a failed allocation holds nothing */
    {
        Buf     a;
        stub::fail_next_alloc = true;
        CHECK(a.alloc(4) == hipErrorOutOfMemory && a.get() == nullptr && a.cap() == 0);
    }
    /* reserve */
    {
        Buf     a;
        bool    replaced = true;
        CHECK(a.reserve(0, 0, nullptr, &replaced) == hipSuccess && !replaced && a.get() == nullptr);
        CHECK(a.reserve(100, 28, nullptr, &replaced) == hipSuccess && replaced && a.cap() == 128);
        void   *const p = a.get();
        /* within the capacity: no call at all */
        stub::log.clear();
        CHECK(a.reserve(128, 1000, nullptr, &replaced) == hipSuccess && !replaced && a.get() == p && a.cap() == 128);
        CHECK(a.reserve(1) == hipSuccess && a.get() == p);
        CHECK(stub::log.empty());
        /* a failure keeps the old pointer and its capacity, and leaves nothing else live */
        stub::fail_next_alloc = true;
        replaced = true;
        CHECK(a.reserve(129, 0, nullptr, &replaced) == hipErrorOutOfMemory && !replaced && a.get() == p && a.cap() == 128);
        CHECK(stub::live.size() == 1 && stub::live.count(p) == 1 && stub::log.empty());
        /* a success allocates first, frees the old pointer exactly once afterwards */
        CHECK(a.reserve(129, 7, nullptr, &replaced) == hipSuccess && replaced && a.cap() == 136);
        CHECK(stub::log == (Log { "alloc", "free" }));
        CHECK(stub::live.size() == 1 && stub::live.count(a.get()) == 1);        /* (p itself may have been handed out again) */
        /* with a drain: allocation, then the drain, then the free */
        ihipStream_t st;
        stub::log.clear();
        CHECK(a.reserve(137, 137, &st) == hipSuccess && a.cap() == 274);
        CHECK(stub::log == (Log { "alloc", "sync", "free" }));
        /* a failure with a drain: the stream is not even drained */
        stub::log.clear();
        stub::fail_next_alloc = true;
        CHECK(a.reserve(275, 0, &st) == hipErrorOutOfMemory && a.cap() == 274 && stub::log.empty());
    }
    CHECK(stub::live.empty());
}

template < typename Own > static void
check_handle(void)
{
    {
        Own     a;
        CHECK(!a);
        CHECK(a.create(0) == hipSuccess && a);
        auto const h = (decltype(+a)) a;
        CHECK(a.create(0) == hipSuccess && (decltype(+a)) a == h && stub::live.size() == 1);     /* made once */
        Own     b(std::move(a));
        CHECK(!a && (decltype(+a)) b == h && stub::live.size() == 1);
        Own     c;
        CHECK(c.create(0) == hipSuccess && stub::live.size() == 2);
        c = std::move(b);
        CHECK(!b && (decltype(+a)) c == h && stub::live.size() == 1);
        std::vector < Own > many;       /* (the windows' events of a batch) */
        for (int i = 0; i < 9; i++) {
            Own     e;
            CHECK(e.create(0) == hipSuccess);
            many.push_back(std::move(e));
        }
        CHECK(stub::live.size() == 10);
        c.release();
        c.release();
        CHECK(!c && stub::live.size() == 9);
    }
    CHECK(stub::live.empty());
}

int
main(void)
{
    check_buffer < LhDevBuf < int > >();
    check_buffer < LhPinned < double > >();
    check_handle < LhEvent > ();
    check_handle < LhStream > ();
    /* the two kinds of memory go back through their own calls (the stand-in aborts on the wrong one) */
    {
        LhDevBuf < char >d;
        LhPinned < char >p;
        CHECK(d.alloc(1) == hipSuccess && p.alloc(1) == hipSuccess);
        CHECK(stub::live[d.get()] == 'd' && stub::live[p.get()] == 'p');
    }
    CHECK(stub::live.empty());
    if (failures)
        fprintf(stderr, "own_check: %d check(s) failed\n", failures);
    else
        printf("own_check: ok\n");
    return failures ? 1 : 0;
}
