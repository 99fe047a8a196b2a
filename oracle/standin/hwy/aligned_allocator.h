// oracle/standin/hwy/aligned_allocator.h -- TEST INFRASTRUCTURE ONLY (see highway.h here): AllocateAligned<T>(n) gives
// an owning pointer to n elements with .get(); the scalar stand-in needs no particular alignment beyond new[]'s.
#pragma once
#include <cstddef>
#include <memory>

namespace hwy {
template <typename T>
std::unique_ptr<T[]> AllocateAligned(size_t n) {
    return std::unique_ptr<T[]>(new T[n]);
}
}  // namespace hwy
