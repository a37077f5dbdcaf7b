// Shared bits of the C-ABI translation units (see include/cuembed_amd.h).
#ifndef CUEMBED_AMD_C_API_COMMON_HPP_
#define CUEMBED_AMD_C_API_COMMON_HPP_

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <iostream>

#include "cuembed_amd.h"

namespace cuembed_c_api {
inline hipStream_t Stream(cuembed_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

template <typename T>
struct TypeTag { using type = T; };

//! From the type codes of a call to its instantiation: call(TypeTag<ElemT>, TypeTag<IndexT>) for (elem_type, index_type),
//! float tables only with kFloatTables.  false: no such instantiation, and the caller's CUEMBED_C_API_BAD_TYPE().
template <bool kFloatTables, typename CallT>
inline bool DispatchTypes(const int elem_type, const int index_type, const CallT& call) {
  const int code = (elem_type << 1) | index_type;   // 0 .. 5: the element code above the index code's one bit
  const auto with_index = [&](auto elem) {
    if ((code & 1) == CUEMBED_I32) call(elem, TypeTag<int32_t>());
    else call(elem, TypeTag<int64_t>());
    return true;
  };
  switch (code >> 1) {
    case CUEMBED_F32:
      if constexpr (kFloatTables) return with_index(TypeTag<float>());
      else return false;
    case CUEMBED_F16: return with_index(TypeTag<__half>());
    case CUEMBED_BF16: return with_index(TypeTag<__hip_bfloat16>());
    default: return false;
  }
}
}  // namespace cuembed_c_api

#define CUEMBED_C_API_BAD_TYPE()                                                     \
  do {                                                                               \
    std::cerr << "Check failed: unsupported type code at " << __FILE__ << ":"        \
              << __LINE__ << std::endl;                                              \
    std::abort();                                                                    \
  } while (0)

#endif  // CUEMBED_AMD_C_API_COMMON_HPP_
