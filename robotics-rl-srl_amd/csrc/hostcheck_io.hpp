// hostcheck_io.hpp — what the case-file host programs (policy_, cnn_policy_, pixel_policy_, pca_project_hostcheck.cpp) share: whole arrays
// in and out of a binary file, and one printed line per verdict of a rule (api_rules.hpp: Verdict).  TESTS ONLY.
#pragma once
#include <stdio.h>

#include <vector>

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}
template <class T> static bool wr(FILE *f, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

template <class V> static void verdict(const char *what, const V &v) { printf("%s: %d %s\n", what, v.code, v.msg ? v.msg : "accepted"); }
