// Host-side helpers every Python-visible entry point goes through before it
// launches. A binding checks metadata only (dtype, sizes, strides, pointer
// alignment, scalar arguments), never tensor contents: per tensor dtype,
// rank, each size, strides; check_on_device last of all, after the scalar
// checks and before any early return, so that a malformed argument is
// reported as itself wherever the tensors live.
#pragma once

#include <torch/extension.h>

#include <initializer_list>
#include <sstream>
#include <type_traits>
#include <utility>

// t must be `dtype` with exactly these sizes (-1: any), contiguous or, with
// unit_inner, a view whose last stride is 1.
inline void check_tensor(const char* op, const at::Tensor& t, const char* name,
                         at::ScalarType dtype, at::IntArrayRef sizes,
                         bool unit_inner = false) {
  bool ok = t.scalar_type() == dtype && t.dim() == (int64_t)sizes.size();
  std::ostringstream want;
  for (size_t d = 0; d < sizes.size(); ++d) {
    ok = ok && (sizes[d] < 0 || t.size(d) == sizes[d]);
    want << (d ? ", " : "");
    if (sizes[d] < 0) want << "?"; else want << sizes[d];
  }
  ok = ok && (unit_inner ? t.dim() == 0 || t.stride(-1) == 1
                         : t.is_contiguous());
  TORCH_CHECK(ok, op, ": ", name, " must be ", dtype, " [", want.str(), "] ",
              unit_inner ? "with unit inner stride" : "contiguous", ", got ",
              t.scalar_type(), " ", t.sizes(), " with strides ", t.strides());
}

// Optional tensor: checked when present; the typed pointer, or nullptr.
template <typename T>
T* check_tensor(const char* op, const c10::optional<at::Tensor>& t,
                const char* name, at::IntArrayRef sizes) {
  if (!t.has_value()) return nullptr;
  check_tensor(op, *t, name, c10::CppTypeToScalarType<T>::value, sizes);
  return t->data_ptr<T>();
}

// The last check of every binding; absent optionals are skipped.
inline void check_on_device(
    const char* op, std::initializer_list<c10::optional<at::Tensor>> ts) {
  for (const auto& t : ts)
    TORCH_CHECK(!t.has_value() || t->is_cuda(), op, ": every tensor must be "
                "on device, got ", t->device(), " for #", &t - ts.begin());
}

// Counts and indices the kernels keep in 32-bit registers.
inline void check_below_2_31(
    const char* op,
    std::initializer_list<std::pair<const char*, int64_t>> values) {
  for (const auto& v : values)
    TORCH_CHECK(v.second >= 0 && v.second < ((int64_t)1 << 31), op, ": ",
                v.first, " must be in [0, 2^31), got ", v.second);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Memory-bound kernels cap the grid and stride over the rest of their work.
constexpr int64_t kMaxStridedGrid = 256 * 8 * 4;
inline dim3 strided_grid(int64_t want) {
  return dim3((unsigned)std::min<int64_t>(want, kMaxStridedGrid));
}

// f(std::integral_constant<int, G>{}) for G == value among Lo, Lo * Step, ..,
// Hi; an error for any other value.
template <int Lo, int Hi, int Step = 2, int G = Lo, typename F>
void dispatch_pow2(const char* op, const char* name, int64_t value, F&& f) {
  if constexpr (G > Hi) {
    TORCH_CHECK(false, op, ": ", name, " must be a power of two in ", Lo, "..",
                Hi, Step == 2 ? "" : " (every second one)", ", got ", value);
  } else if (value == G) {
    f(std::integral_constant<int, G>{});
  } else {
    dispatch_pow2<Lo, Hi, Step, Step * G>(op, name, value, f);
  }
}

// The same error ahead of the launch, for a value the caller passed in.
template <int Lo, int Hi, int Step = 2>
void check_pow2(const char* op, const char* name, int64_t value) {
  dispatch_pow2<Lo, Hi, Step>(op, name, value, [](auto) {});
}

// f(std::true_type{}) or f(std::false_type{}): a bool template argument.
template <typename F>
void dispatch_bool(bool value, F&& f) {
  if (value) f(std::true_type{}); else f(std::false_type{});
}
