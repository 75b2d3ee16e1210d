// The chunk loop of csrc/query_staging.h on the CPU (tests/test_query_staging_cpu.py builds this with -fsanitize=address,undefined and runs it): memcpy is the
// backend, the "device" buffers and the pinned buffer are heap blocks of exactly the size the loop may use, so the sanitizer reports every byte past them.
// One column set per ray-query family; every caller output must hold the record the launch derives from the input record and its global index, every guard
// byte behind a caller array must survive, a column without a caller array must never be copied.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "query_staging.h"

using namespace rt64;

enum Way { DEVICE_ONLY, UP, DOWN };
struct Col { const char *name; Way way; size_t bytes, blocks; };
struct Case { const char *name; std::vector<Col> cols; };

static const size_t GUARD = 48;
static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// byte b of record (k, i) of column c: what the caller puts into its inputs, and what is mixed into every output
static uint8_t pattern(size_t c, size_t k, size_t i, size_t b) { return (uint8_t)((c * 131u + k * 31u + i * 7u + b * 3u + ((i >> 3) * 17u)) ^ 0x5Au); }

static void run(const Case &cs, size_t count, size_t cap) {
    const size_t chunk = std::min(count, cap), C = cs.cols.size();
    size_t first = C;          // the first column that goes up: outputs derive from its block 0
    for (size_t c = 0; c < C; c++) if (cs.cols[c].way == UP && first == C) first = c;
    std::vector<uint8_t *> caller(C, nullptr), device(C, nullptr);
    std::vector<StageColumn> cols(C);
    for (size_t c = 0; c < C; c++) {
        const Col &K = cs.cols[c];
        const size_t bytes = count * K.bytes * K.blocks;
        device[c] = static_cast<uint8_t *>(malloc(chunk * K.bytes * K.blocks));
        memset(device[c], 0xEE, chunk * K.bytes * K.blocks);
        if (K.way != DEVICE_ONLY) {
            caller[c] = static_cast<uint8_t *>(malloc(bytes + GUARD));
            memset(caller[c], 0xAB, bytes + GUARD);
            if (K.way == UP) for (size_t k = 0; k < K.blocks; k++) for (size_t i = 0; i < count; i++) for (size_t b = 0; b < K.bytes; b++)
                caller[c][(k * count + i) * K.bytes + b] = pattern(c, k, i, b);
        }
        cols[c] = StageColumn{K.way == UP ? caller[c] : nullptr, K.way == DOWN ? caller[c] : nullptr, device[c], K.bytes, K.blocks};
    }
    const size_t pinBytes = stage_pin_bytes(cols.data(), C, chunk);
    size_t upB = 0, downB = 0;
    for (const Col &K : cs.cols) { if (K.way == UP) upB += K.bytes * K.blocks; if (K.way == DOWN) downB += K.bytes * K.blocks; }
    EXPECT(pinBytes == chunk * std::max(upB, downB), "%s: pin buffer of %zu bytes", cs.name, pinBytes);
    uint8_t *pin = static_cast<uint8_t *>(malloc(pinBytes ? pinBytes : 1));
    int phase = 3;          // 0 up copies, 1 launched, 2 down copies, 3 waited
    size_t next = 0, launches = 0, n_now = 0;
    auto column_of = [&](const void *d) { size_t c = 0; while (c < C && device[c] != d) c++; return c; };
    auto up = [&](void *d, const void *p, size_t bytes) {
        const size_t c = column_of(d);
        EXPECT(c < C && cs.cols[c].way == UP, "%s: an up copy into a column that does not go up", cs.name);
        EXPECT(phase == 3 || phase == 0, "%s: an up copy in phase %d", cs.name, phase);
        EXPECT(static_cast<const uint8_t *>(p) >= pin && static_cast<const uint8_t *>(p) + bytes <= pin + pinBytes, "%s: an up copy from outside the pin buffer", cs.name);
        phase = 0; memcpy(d, p, bytes);
    };
    auto launch = [&](size_t at, size_t n) {
        EXPECT(at == next && n == std::min(chunk, count - at) && n > 0, "%s: launch(%zu, %zu), expected at %zu", cs.name, at, n, next);
        EXPECT(phase == (upB ? 0 : 3), "%s: a launch in phase %d", cs.name, phase);
        phase = 1; next = at + n; launches++; n_now = n;
        for (size_t c = 0; c < C; c++) {
            const Col &K = cs.cols[c];
            for (size_t k = 0; k < K.blocks; k++) for (size_t i = 0; i < n; i++) for (size_t b = 0; b < K.bytes; b++) {
                uint8_t &x = device[c][(k * n + i) * K.bytes + b];
                if (K.way == UP) EXPECT(x == pattern(c, k, at + i, b), "%s: column %s record (%zu, %zu) byte %zu on the device", cs.name, K.name, k, at + i, b);
                else x = pattern(c, k, at + i, b) ^ (first < C ? device[first][i * cs.cols[first].bytes + b % cs.cols[first].bytes] : 0);
            }
        }
    };
    auto down = [&](void *p, const void *d, size_t bytes) {
        const size_t c = column_of(d);
        EXPECT(c < C && cs.cols[c].way == DOWN, "%s: a down copy from a column that does not come down", cs.name);
        EXPECT(phase == 1 || phase == 2, "%s: a down copy in phase %d", cs.name, phase);
        EXPECT(c < C && bytes == n_now * cs.cols[c].bytes * cs.cols[c].blocks, "%s: a down copy of %zu bytes", cs.name, bytes);
        EXPECT(static_cast<uint8_t *>(p) >= pin && static_cast<uint8_t *>(p) + bytes <= pin + pinBytes, "%s: a down copy to outside the pin buffer", cs.name);
        phase = 2; memcpy(p, d, bytes);
    };
    auto wait = [&] { EXPECT(phase == (downB ? 2 : 1), "%s: a wait in phase %d", cs.name, phase); phase = 3; };
    stage_chunks(cols.data(), C, count, cap, pin, up, launch, down, wait);
    EXPECT(next == count && launches == (count + cap - 1) / cap && phase == 3, "%s: %zu launches reached %zu of %zu", cs.name, launches, next, count);
    for (size_t c = 0; c < C; c++) {
        const Col &K = cs.cols[c];
        if (K.way == DEVICE_ONLY) continue;
        const size_t bytes = count * K.bytes * K.blocks;
        for (size_t k = 0; k < K.blocks; k++) for (size_t i = 0; i < count; i++) for (size_t b = 0; b < K.bytes; b++) {
            uint8_t want = pattern(c, k, i, b);
            if (K.way == DOWN && first < C) want ^= pattern(first, 0, i, b % cs.cols[first].bytes);
            EXPECT(caller[c][(k * count + i) * K.bytes + b] == want, "%s count %zu: column %s record (%zu, %zu) byte %zu", cs.name, count, K.name, k, i, b);
        }
        for (size_t g = 0; g < GUARD; g++) EXPECT(caller[c][bytes + g] == 0xAB, "%s count %zu: guard byte %zu behind column %s", cs.name, count, g, K.name);
    }
    for (size_t c = 0; c < C; c++) { free(caller[c]); free(device[c]); }
    free(pin);
}

static Case layers(const char *name, size_t L) { return {name, {{"rays", UP, 32, 1}, {"hits", DOWN, 32, L}, {"lods", UP, 4, 1}, {"layers", DOWN, 16, 1}, {"weights", DOWN, 4, L}, {"coverage", DOWN, 16, 1}}}; }
static Case weigh(const char *name, size_t L) { return {name, {{"rays", UP, 32, 1}, {"hits", UP, 32, L}, {"lods", UP, 4, 1}, {"weights", DOWN, 4, L}, {"coverage", DOWN, 16, 1}}}; }

int main(int argc, char **argv) {
    const size_t cap = argc > 1 ? (size_t)atoi(argv[1]) : 7;
    const std::vector<Case> cases = {
        {"trace", {{"rays", UP, 32, 1}, {"hits", DOWN, 32, 1}}},
        {"trace + resolve, hits = NULL", {{"rays", UP, 32, 1}, {"hits", DEVICE_ONLY, 32, 1}, {"lods", UP, 4, 1}, {"records", DOWN, 64, 1}}},
        {"pixel footprints", {{"pixels", UP, 8, 1}, {"rays", DOWN, 32, 1}, {"diffs", DEVICE_ONLY, 64, 1}, {"hits", DOWN, 32, 1}, {"footprints", DOWN, 64, 1}}},
        {"pixel footprints, rays = hits = NULL", {{"pixels", UP, 8, 1}, {"rays", DEVICE_ONLY, 32, 1}, {"diffs", DEVICE_ONLY, 64, 1}, {"hits", DEVICE_ONLY, 32, 1}, {"footprints", DOWN, 64, 1}}},
        {"pixel footprints, pixels = NULL", {{"rays", DOWN, 32, 1}, {"diffs", DEVICE_ONLY, 64, 1}, {"hits", DEVICE_ONLY, 32, 1}, {"footprints", DOWN, 64, 1}}},
        {"bounces, reflected only", {{"rays", UP, 32, 1}, {"hits", DEVICE_ONLY, 32, 1}, {"lods", UP, 4, 1}, {"reflected", DOWN, 32, 1}}},
        {"chains, depth 8", {{"rays", UP, 32, 1}, {"hits", DOWN, 32, 8}, {"lods", UP, 4, 1}, {"bounces", DOWN, 32, 8}}},
        layers("layers, walk + weigh, 16", 16), layers("layers, walk + weigh, 3", 3), weigh("weigh alone, 16", 16), weigh("weigh alone, 3", 3),
    };
    size_t runs = 0;
    for (const Case &cs : cases) for (size_t count : {(size_t)1, cap - 1, cap, cap + 1, 3 * cap + 2}) if (count) { run(cs, count, cap); runs++; }
    printf("%zu runs, cap %zu, %d failures\n", runs, cap, failures);
    return failures ? 1 : 0;
}
