// ebvo_carve.h -- the layout of a carved buffer: arrays one after another, each starting on a multiple of 64 bytes.
// Host-only and free of HIP: offsets are computed first, the buffer is grown to total() afterwards.
#pragma once
#include <cstddef>

// the next multiple of 64 bytes: where the next array of a carved workspace starts
inline size_t round_up64(size_t v) { return (v + 63) & ~(size_t)63; }

struct Carve
{
    size_t end = 0;

    // the offset of an array of `bytes` bytes (an empty one shares its offset with the next)
    size_t take(size_t bytes)
    {
        const size_t at = end;
        end = round_up64(end + bytes);
        return at;
    }
    size_t total() const { return end; } // the bytes to allocate
};
