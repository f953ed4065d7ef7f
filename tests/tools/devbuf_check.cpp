// Stand-alone driver of the owning device buffer (nexoclom_amd/csrc/nxc_devbuf.hpp) over a fake
// allocator: malloc memory, so that the host sanitizers see a block freed twice or never; counters
// of live blocks and of every alloc, free and flush; and orders to refuse the next n allocations or
// the next free.  A refused free still gives the block back -- what is under test is that DevBuf
// forgets the pointer, never that memory is lost.  Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/devbuf_check.cpp -o devbuf_check && ./devbuf_check
// Prints one line per case; exit status 0 when every case went as expected and no block outlived
// its scope.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../nexoclom_amd/csrc/nxc_devbuf.hpp"

namespace {

constexpr int REFUSED = 7;           // the fake's error status

struct Fake {
    static inline int live = 0, allocs = 0, frees = 0, flushes = 0;
    static inline size_t last_bytes = 0;
    static inline int fail_allocs = 0;       // refuse this many allocations from now on
    static inline bool fail_free = false;    // refuse (report) the next free
    static int alloc(void **ptr, size_t bytes)
    {
        allocs++;
        if (fail_allocs > 0) { fail_allocs--; return REFUSED; }
        *ptr = std::malloc(bytes);
        last_bytes = bytes;
        live++;
        return 0;
    }
    static int free(void *ptr)
    {
        frees++;
        std::free(ptr);
        live--;
        if (fail_free) { fail_free = false; return REFUSED; }
        return 0;
    }
    static int flush() { flushes++; return 0; }
    static void reset() { allocs = frees = flushes = 0; fail_allocs = 0; fail_free = false; }
};
using Buf = DevBuf<double, Fake>;

int unexpected = 0;

void check(const char *name, bool ok)
{
    std::printf("%s%s\n", name, ok ? " ok" : " -- UNEXPECTED");
    if (!ok) unexpected++;
}
bool calls(int allocs, int frees, int flushes)
{
    return Fake::allocs == allocs && Fake::frees == frees && Fake::flushes == flushes;
}
// what every case ends with: its buffers are out of scope
void scope_exit(const char *name) { check(name, Fake::live == 0); }

void grow_and_keep()
{
    {
        Buf b;
        Fake::reset();
        check("new buffer is empty", !b && b.get() == nullptr && b.cap == 0);
        check("ensure(100) allocates once", b.ensure(100) == 0 && b && b.cap == 100 && calls(1, 0, 0) &&
                                                Fake::last_bytes == 100);
        double *p = b;
        Fake::reset();
        check("ensure(50) keeps the block", b.ensure(50) == 0 && b.get() == p && b.cap == 100 && calls(0, 0, 0));
        check("ensure(100) keeps the block", b.ensure(100) == 0 && b.get() == p && b.cap == 100 && calls(0, 0, 0));
        check("ensure(101) frees once and allocates once",
              b.ensure(101) == 0 && b && b.cap == 101 && calls(1, 1, 0) && Fake::live == 1);
        check("the pointer converts and offsets", b + 3 == b.get() + 3);
    }
    {
        Buf b;
        Fake::reset();
        check("ensure(0) allocates 8 bytes, capacity 0",
              b.ensure(0) == 0 && b && b.cap == 0 && calls(1, 0, 0) && Fake::last_bytes == 8);
        double *p = b;
        check("a second ensure(0) makes no call", b.ensure(0) == 0 && b.get() == p && calls(1, 0, 0));
    }
    scope_exit("grow and keep: no block left");
}

void failed_allocation()
{
    {
        Buf b;
        Fake::reset();
        Fake::fail_allocs = 1;
        check("one refused allocation: one flush, the retry succeeds",
              b.ensure(64) == 0 && b && b.cap == 64 && calls(2, 0, 1));
        Fake::reset();
        Fake::fail_allocs = 2;
        check("two refused allocations: the error, the buffer empty",
              b.ensure(128) == REFUSED && !b && b.cap == 0 && calls(2, 1, 1) && Fake::live == 0);
        Fake::reset();
        check("the next ensure succeeds, nothing is freed again",
              b.ensure(128) == 0 && b && b.cap == 128 && calls(1, 0, 0) && Fake::live == 1);
    }
    scope_exit("failed allocation: no block left");
}

void failed_free()
{
    {
        Buf b;
        (void)b.ensure(16);
        Fake::reset();
        Fake::fail_free = true;
        check("a refused free inside ensure: the error, the buffer empty, nothing allocated",
              b.ensure(32) == REFUSED && !b && b.cap == 0 && calls(0, 1, 0));
        Fake::reset();
        check("release after it makes no free call", b.release() == 0 && calls(0, 0, 0));
    }
    check("the destructor after it makes no free call", calls(0, 0, 0));
    {
        Buf b;
        (void)b.ensure(16);
        Fake::reset();
        Fake::fail_free = true;
        check("a refused free inside release: the error, the buffer empty",
              b.release() == REFUSED && !b && b.cap == 0 && calls(0, 1, 0));
        Fake::reset();
        check("a later release makes no free call", b.release() == 0 && calls(0, 0, 0));
    }
    check("the destructor after it makes no free call", calls(0, 0, 0));
    scope_exit("failed free: no block left");
}

void release_and_move()
{
    {
        Buf b;
        (void)b.ensure(24);
        Fake::reset();
        check("release twice makes one free", b.release() == 0 && b.release() == 0 && !b && calls(0, 1, 0));
    }
    {
        Buf a;
        (void)a.ensure(40);
        double *p = a;
        Fake::reset();
        Buf b(std::move(a));
        check("move-construct: the source is empty, no allocator call",
              !a && a.cap == 0 && b.get() == p && b.cap == 40 && calls(0, 0, 0));
        Buf c;
        (void)c.ensure(8);
        Fake::reset();
        c = std::move(b);
        check("move-assign: the source is empty, the overwritten block freed once",
              !b && b.cap == 0 && c.get() == p && c.cap == 40 && calls(0, 1, 0) && Fake::live == 1);
        Buf &same = c;
        c = std::move(same);
        check("move-assign to itself keeps the block", c.get() == p && c.cap == 40 && calls(0, 1, 0));
    }
    scope_exit("release and move: no block left");
}

}  // namespace

int main()
{
    grow_and_keep();
    failed_allocation();
    failed_free();
    release_and_move();
    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
