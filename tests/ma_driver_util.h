// What the host drivers of the ma bodies (tests/ma_*_driver.cpp) share: arrays the sanitizer sees every index of, and a line reader.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

template <class T>
struct Exact {                              // exactly `count` elements on the heap (none: a null pointer)
  T* p = nullptr;
  explicit Exact(size_t count, size_t align = alignof(T)) {
    if (!count) return;
    const size_t bytes = count * sizeof(T);                  // (an aligned block's size is a multiple of its alignment: the caller's)
    p = (T*)(align > alignof(T) ? aligned_alloc(align, bytes) : malloc(bytes));
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, 0, bytes);
  }
  ~Exact() { free(p); }
  Exact(const Exact&) = delete;
  Exact& operator=(const Exact&) = delete;
};

inline std::string line_of(FILE* f) {
  std::string s;
  int ch;
  while ((ch = fgetc(f)) != EOF && ch != '\n') s += (char)ch;
  return s;
}
