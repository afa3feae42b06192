// rng.h — the counter hash behind the library's stateless generators: a value is a function of (seed, index) alone, so no
// generator state is stored or advanced and any thread can produce any element.  Users: normal_at (augment.hip), the elastic
// field's noise (warp.hip).
#pragma once
#include <stdint.h>

// splitmix64's output function on x + golden ratio
__host__ __device__ __forceinline__ uint64_t mix64a(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
