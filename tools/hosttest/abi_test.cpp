// include/mp2g.h as the C++ front end reads it, for the Python host's ctypes table and structure mirrors to be held against
// (tests/test_abi_prototypes.py writes the two lists from them). No GPU, no library: nothing of mp2g.h is called or linked.
// build: hipcc -x hip --cuda-host-only -O2 -std=c++17 -I../../include -I<dir of the lists> abi_test.cpp -o abi_test
//   abi_funcs.inc   one X(name) per function   -> "F name n_args ret arg...", each of them p (pointer), v (void) or <bytes><s|u>
//   abi_structs.inc S(type), then M(type, field) per field -> "S type sizeof", "M type field offsetof sizeof"
#include "mp2g.h"
#include <cstddef>
#include <cstdio>
#include <type_traits>

template <class T> static void kind() {
  if constexpr (std::is_void_v<T>) printf(" v");
  else if constexpr (std::is_pointer_v<T>) printf(" p");
  else {
    static_assert(std::is_integral_v<T>, "mp2g.h passes pointers and integers only");
    printf(" %zu%c", sizeof(T), std::is_signed_v<T> ? 's' : 'u');
  }
}

template <class F> struct Sig;
template <class R, class... A> struct Sig<R (*)(A...)> {
  static void print(const char* name) {
    printf("F %s %zu", name, sizeof...(A));
    kind<R>();
    (kind<A>(), ...);
    printf("\n");
  }
};

int main() {
#define X(name) Sig<decltype(&name)>::print(#name);
#include "abi_funcs.inc"
#define S(type) printf("S " #type " %zu\n", sizeof(type));
#define M(type, field) printf("M " #type " " #field " %zu %zu\n", offsetof(type, field), sizeof(((type*)nullptr)->field));
#include "abi_structs.inc"
  return 0;
}
