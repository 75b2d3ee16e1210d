// query_staging.h -- the chunk loop behind every host-array ray query (rt64_host.cpp, run_view_*).
//
// A call's arrays are columns of records.  Chunk by chunk the loop gathers the columns that go up into one pinned buffer and copies them to their device buffers,
// lets the caller launch its kernels, copies the columns that come down back into the pinned buffer, waits once, and scatters them to the caller's arrays.
// The device side arrives as four callables, so this header needs no HIP: rt64_host.cpp passes hipMemcpyAsync and a stream wait, tests/query_staging_probe.cpp memcpy.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace rt64 {

struct StageColumn {
    const void *src;      // the caller's array that goes up, or NULL
    void *dst;            // the caller's array that comes down, or NULL (both NULL: the column lives on the device only and is never read, copied or written here)
    void *dev;            // device buffer of chunk * bytes * blocks
    size_t bytes;         // one record
    size_t blocks;        // 1, or depth / maxLayers: record (k, i) sits at k * count + i in the caller's array and at k * n + i in a chunk of n
};

// The pinned buffer a chunk needs: the columns going up share it, then the columns coming down.
inline size_t stage_pin_bytes(const StageColumn *cols, size_t columns, size_t chunk) {
    size_t up = 0, down = 0;
    for (size_t c = 0; c < columns; c++) { if (cols[c].src) up += cols[c].bytes * cols[c].blocks; if (cols[c].dst) down += cols[c].bytes * cols[c].blocks; }
    return chunk * std::max(up, down);
}

// One round trip per chunk of at most `chunk` records: up(dev, pin, bytes) per column in order, launch(at, n) -- records at .. at + n - 1 of the call are records
// 0 .. n - 1 of every device buffer --, down(pin, dev, bytes) per column in order, wait().  `pin` holds stage_pin_bytes(cols, columns, min(chunk, count)).
template <class Up, class Launch, class Down, class Wait>
void stage_chunks(const StageColumn *cols, size_t columns, size_t count, size_t chunk, uint8_t *pin, Up &&up, Launch &&launch, Down &&down, Wait &&wait) {
    for (size_t at = 0; at < count; at += chunk) {
        const size_t n = std::min(chunk, count - at);
        uint8_t *p = pin;
        for (size_t c = 0; c < columns; c++) {
            const StageColumn &C = cols[c];
            if (!C.src) continue;
            for (size_t k = 0; k < C.blocks; k++) memcpy(p + k * n * C.bytes, static_cast<const uint8_t *>(C.src) + (k * count + at) * C.bytes, n * C.bytes);
            up(C.dev, p, n * C.bytes * C.blocks); p += n * C.bytes * C.blocks;
        }
        launch(at, n);
        p = pin;
        for (size_t c = 0; c < columns; c++) if (cols[c].dst) { down(p, cols[c].dev, n * cols[c].bytes * cols[c].blocks); p += n * cols[c].bytes * cols[c].blocks; }
        wait();
        p = pin;
        for (size_t c = 0; c < columns; c++) {
            const StageColumn &C = cols[c];
            if (!C.dst) continue;
            for (size_t k = 0; k < C.blocks; k++) memcpy(static_cast<uint8_t *>(C.dst) + (k * count + at) * C.bytes, p + k * n * C.bytes, n * C.bytes);
            p += n * C.bytes * C.blocks;
        }
    }
}

}  // namespace rt64
