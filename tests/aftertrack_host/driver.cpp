// track_commit_host (dsdtm_amd/host/dsdtm_slam_host.hpp: plain C++, no device call, no library) on the cases
// tests/test_aftertrack_cpu.py writes; the answers go back as a flat binary file that the test holds against the restatement, byte for
// byte. One job per map: its descs run in order on the map as the earlier ones left it.
// Build: g++ -O2 -std=c++14 -ffp-contract=off. Usage: driver <cases.bin> <answers.bin>
#include <cstdio>
#include <cstdlib>

#include "../../dsdtm_amd/host/dsdtm_slam_host.hpp"

static FILE* in;
static FILE* out;

template <class T>
static std::vector<T> take(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
template <class T>
static void put(const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), out); }
static void put_int(int32_t v) { fwrite(&v, 4, 1, out); }

int main(int argc, char** argv) {
    if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 1;
    const int32_t n_jobs = take<int32_t>(1)[0];
    for (int32_t job = 0; job < n_jobs; ++job) {
        const std::vector<int32_t> head = take<int32_t>(2);
        const size_t P = (size_t)head[0], K = (size_t)head[1];
        std::vector<int32_t> found = take<int32_t>(P);
        std::vector<uint8_t> bad = take<uint8_t>(P);
        const std::vector<int32_t> n_slots = take<int32_t>(K);
        size_t S = 0;
        for (size_t k = 0; k < K; ++k) S += (size_t)n_slots[k];
        std::vector<int32_t> slots = take<int32_t>(S);
        std::vector<uint8_t> observes = take<uint8_t>(S);
        const double threshold = take<double>(1)[0];
        DSDTM::TrackCommitMap m;
        m.n_points = (int32_t)P; m.found = found.data(); m.bad = bad.data();
        m.n_slots_total = (int64_t)S; m.point_of_slot = slots.data(); m.observes = observes.data();
        const int32_t n_descs = take<int32_t>(1)[0];
        for (int32_t t = 0; t < n_descs; ++t) {
            const int32_t n = take<int32_t>(1)[0];
            const std::vector<int32_t> point = take<int32_t>((size_t)n);
            const std::vector<double> norm = take<double>((size_t)n);
            const DSDTM::TrackCommitHost r = DSDTM::track_commit_host(m, threshold, n, point.data(), norm.data());
            put_int(r.n_erased); put_int((int32_t)r.bad_points.size());
            put(r.bad_points); put(r.found_after);
        }
        put(found); put(bad); put(slots); put(observes);        // the map after the descs
    }
    fclose(out);
    return 0;
}
