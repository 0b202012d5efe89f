// The layout of one packed block: the arrays an entry point sends to the device and brings back, one behind the other, each at a multiple of
// 256 bytes.  Plain C++ without a HIP header, so a host program can include it (tests/cpp/blob_layout_host.cpp).  The transfers of such a block
// are ygz_blob_open / ygz_blob_upload / ygz_blob_fetch (ygz_internal.h, ctx.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

inline size_t ygz_round_up_256(size_t x) { return (x + 255) & ~(size_t)255; }

struct YgzBlobLayout {
    static constexpr size_t BAD = SIZE_MAX;       // no multiple of 256: never the end of a good layout
    size_t end = 0;                               // bytes so far; read it between two add()s to mark where the upload or the copy back ends
    bool bad() const { return end == BAD; }       // a size overflowed size_t; stays bad, and ygz_blob_open refuses it
    // the offset of the next array of `bytes` bytes; add(0) returns end and leaves it (an optional array that is absent)
    size_t add(size_t bytes)
    {
        const size_t at = end;
        if (bad() || bytes > SIZE_MAX - 255 - end) end = BAD;
        else end = ygz_round_up_256(end + bytes);
        return at;
    }
    // add(count * sizeof(T)); that multiplication is the one checked.  The count is the caller's own product of validated ints, formed in
    // size_t, and is not checked here: callers pass elements, not bytes, so that the element size never hides in an unchecked product
    template <class T> size_t add_n(size_t count)
    {
        if (count > SIZE_MAX / sizeof(T)) { end = BAD; return end; }
        return add(count * sizeof(T));
    }
};
