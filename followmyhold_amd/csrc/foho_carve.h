// foho_carve.h -- the bump allocator of every workspace layout (host only).
#pragma once
#include <stddef.h>

// Byte offsets from 0, every block rounded up to 256 bytes; `off` is the running offset and ends as the layout's total.
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
};
