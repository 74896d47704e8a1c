// Stand-alone check of the field lists of the C ABI's optional stages (csrc/io_fields.hpp): every IO block is carved from a
// heap block of exactly the size the null-base pass gave, every array is written over its full extent with a pattern of its
// own, and the generic copier carries inputs and outputs into heap blocks of exactly each array's size.  Built with
// -fsanitize=address,undefined by tests/test_io_fields_native_cpu.py and run as a program of its own (no GPU, nothing loaded
// into python); exit status 0 = every check passed, and a count that is off by one element is an ASan report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../low-cost-mocap_amd/csrc/io_fields.hpp"

static int failures = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                              \
    }                                                          \
  } while (0)

// the byte every position of array number `field` holds
static unsigned char pattern(int field, size_t i) { return (unsigned char)(31 * (field + 1) + 7 * i); }

template <class IO>
static void check_block(IO io, const IoDims& n, int n_fields, int n_inputs) {
  // 1. the null-base pass sizes the block, the second pass hands out pointers inside it
  IO sized = io;
  Carver c0(nullptr);
  carve(c0, sized, n);
  const size_t total = c0.off;
  unsigned char* block = (unsigned char*)malloc(total ? total : 1);
  Carver c(block);
  carve(c, io, n);
  CHECK(c.off == total);
  // 2. every array written over its full extent (inside the block, past no other array: ASan and the patterns say so)
  int field = 0, inputs = 0;
  std::vector<size_t> bytes;
  IO::fields(n, [&](auto m, size_t count) {
    using T = std::remove_pointer_t<std::remove_reference_t<decltype(io.*m)>>;
    unsigned char* p = (unsigned char*)(io.*m);
    CHECK(p >= block && p + sizeof(T) * count <= block + total);
    CHECK((uintptr_t)p % alignof(T) == 0);
    for (size_t i = 0; i < sizeof(T) * count; i++) p[i] = pattern(field, i);
    bytes.push_back(sizeof(T) * count);
    inputs += std::is_const_v<T>;
    field++;
  });
  CHECK(field == n_fields && inputs == n_inputs);
  // 3. destinations of exactly each array's size; inputs and outputs travel separately and each lands where it belongs
  IO dst = io;
  std::vector<void*> owned;
  field = 0;
  IO::fields(n, [&](auto m, size_t) {
    using T = std::remove_const_t<std::remove_pointer_t<std::remove_reference_t<decltype(dst.*m)>>>;
    void* p = bytes[field] ? calloc(bytes[field], 1) : nullptr;  // (an array of no elements may be null: it is never touched)
    owned.push_back(p);
    dst.*m = (T*)p;
    field++;
  });
  size_t copied = 0;
  auto counting_copy = [&](void* d, const void* s, size_t b) {
    copied += b;
    return HostCopy{}(d, s, b);
  };
  CHECK(copy_fields<false>(dst, io, n, counting_copy) == 0);
  field = 0;
  size_t want = 0;
  int outputs_with_elements = 0;
  IO::fields(n, [&](auto m, size_t) {
    using T = std::remove_pointer_t<std::remove_reference_t<decltype(io.*m)>>;
    const unsigned char* p = (const unsigned char*)(dst.*m);
    for (size_t i = 0; i < bytes[field]; i++) CHECK(p[i] == (std::is_const_v<T> ? 0 : pattern(field, i)));  // inputs not yet
    if (!std::is_const_v<T>) want += bytes[field];
    outputs_with_elements += !std::is_const_v<T> && bytes[field];
    field++;
  });
  CHECK(copied == want);
  CHECK(copy_fields<true>(dst, io, n, counting_copy) == 0);
  field = 0;
  IO::fields(n, [&](auto m, size_t) {
    const unsigned char* p = (const unsigned char*)(dst.*m);
    for (size_t i = 0; i < bytes[field]; i++) CHECK(p[i] == pattern(field, i));
    want += std::is_const_v<std::remove_pointer_t<std::remove_reference_t<decltype(io.*m)>>> ? bytes[field] : 0;
    field++;
  });
  CHECK(copied == want);
  // 4. a copier that fails ends the copying and its code comes back
  int calls = 0;
  const int rc = copy_fields<false>(dst, io, n, [&](void*, const void*, size_t) { return ++calls == 2 ? -7 : 0; });
  CHECK(outputs_with_elements >= 2 ? (rc == -7 && calls == 2) : (rc == 0 && calls == outputs_with_elements));
  for (void* p : owned) free(p);
  free(block);
}

int main() {
  for (size_t F : {1, 3})
    for (size_t K : {1, 64})
      for (size_t B : {0, 1, 3})
        for (size_t D : {1, 4}) {
          const IoDims n{F, K, B, D};
          check_block(FilterIO{}, n, 5, 1);
          check_block(BodiesIO{(int)B}, n, 8, 0);
          check_block(MarkersIO{}, n, 5, 1);
        }
  // the element counts themselves, against the shapes include/mocap_core.h documents
  const IoDims n{3, 64, 2, 4};
  std::vector<size_t> got;
  auto note = [&](auto, size_t count) { got.push_back(count); };
  FilterIO::fields(n, note);
  CHECK((got == std::vector<size_t>{3, 3 * 4 * 3, 3 * 4 * 3, 3 * 4, 3 * 4}));
  got.clear();
  BodiesIO::fields(n, note);
  CHECK((got == std::vector<size_t>{6, 6, 6 * 8, 6 * 9, 6 * 3, 6, 6, 6}));
  got.clear();
  MarkersIO::fields(n, note);
  CHECK((got == std::vector<size_t>{3, 3 * 64, 3 * 64, 3, 3}));
  // ... and the degenerate shapes: no body slots, one filtered object, one point per frame
  const IoDims m{1, 1, 0, 1};
  got.clear();
  FilterIO::fields(m, note);
  CHECK((got == std::vector<size_t>{1, 3, 3, 1, 1}));
  got.clear();
  BodiesIO::fields(m, note);
  CHECK((got == std::vector<size_t>{0, 0, 0, 0, 0, 0, 0, 0}));
  got.clear();
  MarkersIO::fields(m, note);
  CHECK((got == std::vector<size_t>{1, 1, 1, 1, 1}));
  const IoDims b3{2, 5, 3, 1};
  got.clear();
  BodiesIO::fields(b3, note);
  CHECK((got == std::vector<size_t>{6, 6, 48, 54, 18, 6, 6, 6}));
  if (failures) return 1;
  printf("io field checks ok\n");
  return 0;
}
