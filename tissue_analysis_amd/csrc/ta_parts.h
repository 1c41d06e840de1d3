// ta_parts.h -- the parts of a device buffer (plain host C++, no HIP: tests/native/parts.cpp compiles it on its own).  A buffer that
// holds several arrays is laid out by a cursor that hands out one part after the other; a layout struct names its parts and fills
// them through the cursor, so each line states its own size, and the memset, the kernel arguments and the getter take offset and
// size from the part.
#pragma once
#include <cstdint>

struct Part {
    uint64_t at = 0, bytes = 0;                         // byte offset from the buffer's base, size
};

struct PartCursor {
    uint64_t at;
    constexpr explicit PartCursor(uint64_t from = 0) : at(from) {}
    // the next `bytes`, from the next multiple of `align` (a power of two or not; 1 = where the last part ended)
    constexpr Part take(uint64_t bytes, uint64_t align = 1) {
        const Part p = {end(align), bytes};
        at = p.at + bytes;
        return p;
    }
    // the bytes handed out so far, padded to a multiple of `align`: the size of the buffer
    constexpr uint64_t end(uint64_t align = 1) const { return (at + align - 1) / align * align; }
};
