// glm/gtc/constants.hpp of the GLM STAND-IN (see ../glm.hpp: test infrastructure, not GLM).
#pragma once
#include "../glm.hpp"

namespace glm {

// gtc/constants.inl: pi<T>() = static_cast<T>(3.14159265358979323846264338327950288)
template <typename T>
constexpr T pi() { return static_cast<T>(3.14159265358979323846264338327950288); }

}  // namespace glm
