// carve_check.cpp -- csrc/ebvo_carve.h on its own (host compiler, no HIP): every array of a carved buffer starts on a multiple
// of 64 bytes, consecutive arrays do not overlap, total() covers the last one, and nothing wraps a size_t.
//   g++ -std=c++17 -O2 -Wall -Werror -I edge_based_visual_odometry_amd/csrc tests/cpp/carve_check.cpp -o carve_check
//   ./carve_check [bytes of one ebvo_edge, default 32]
#include "ebvo_carve.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;

static void expect(bool ok, const char *what, size_t a, size_t b)
{
    if (ok)
        return;
    if (++failures <= 10)
        std::printf("FAIL %s (%zu, %zu)\n", what, a, b);
}

// carve the arrays of `bytes` in order and check the layout against a sum formed in 128 bits
static void check(const std::vector<size_t> &bytes)
{
    Carve L;
    unsigned __int128 want = 0; // where the next array has to start
    size_t prev_end = 0;
    for (size_t b : bytes)
    {
        const size_t at = L.take(b);
        expect(at % 64 == 0, "offset is a multiple of 64", at, b);
        expect(at >= prev_end, "the array starts behind the one before it", at, prev_end);
        expect((unsigned __int128)at == want, "offset equals the unwrapped sum", at, b);
        expect(at + b >= at, "offset + size does not wrap", at, b);
        expect(L.total() >= at + b, "total() covers the array", L.total(), at + b);
        expect(L.total() % 64 == 0 && L.total() - (at + b) < 64, "total() is the next multiple of 64", L.total(), at + b);
        prev_end = at + b;
        want += ((unsigned __int128)b + 63) / 64 * 64;
    }
    expect((unsigned __int128)L.total() == want, "total() equals the unwrapped sum", L.total(), (size_t)want);
}

int main(int argc, char **argv)
{
    static_assert(sizeof(size_t) == 8, "the layouts of the library are 64-bit");
    const size_t edge = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 32;
    const size_t counts[] = {0, 1, 3, 63, 64, 65, 2147483647u}, sizes[] = {1, 4, 8, edge};
    std::vector<size_t> all;
    for (size_t c : counts)
        for (size_t s : sizes)
            all.push_back(c * s);
    expect(Carve().total() == 0 && round_up64(0) == 0 && round_up64(1) == 64 && round_up64(64) == 64 && round_up64(65) == 128,
           "round_up64 and the empty layout", 0, 0);
    check(all); // every array once, in one buffer
    for (size_t a : all) // every ordered pair, and the pair between two sentinel elements as the entry points pad their lists
        for (size_t b : all)
        {
            check({a, b});
            check({edge, a, b, edge});
        }
    if (failures)
    {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok: %zu arrays, %zu ordered pairs\n", all.size(), all.size() * all.size());
    return 0;
}
