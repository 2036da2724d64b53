// make pose_topk_host_check: the selection of pose_topk.h on the host under ASan + UBSan, against std::sort.
// Random and tie-heavy inputs (cosines drawn from a handful of values, so that the index decides most ranks); insert alone,
// then the two-level use of the kernels: partial lists of interleaved subsets, merged in a fixed order.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

#include "pose_topk.h"

namespace {

using Entry = std::pair<double, int32_t>;

std::vector<Entry> oracle(std::vector<Entry> v, int k) {
    std::sort(v.begin(), v.end(), [](const Entry& a, const Entry& b) { return pose_before(a.first, a.second, b.first, b.second); });
    v.resize(k, Entry(pose_topk_neg_inf(), POSE_TOPK_EMPTY));
    return v;
}

template <int K>
bool same(const PoseTopK<K>& t, const std::vector<Entry>& want, const char* what, int n) {
    for (int j = 0; j < K; ++j)
        if (t.i[j] != want[j].second || !(t.c[j] == want[j].first)) {
            std::fprintf(stderr, "pose_topk_host_check: %s K=%d n=%d slot %d: got (%.17g, %d), want (%.17g, %d)\n", what, K, n, j,
                         t.c[j], t.i[j], want[j].first, want[j].second);
            return false;
        }
    return true;
}

template <int K>
bool run(std::mt19937_64& rng, int n, int levels) {
    std::vector<Entry> v(n);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (int j = 0; j < n; ++j) {
        const double c = levels ? std::floor(u(rng) * levels) / levels : u(rng);
        v[j] = Entry(c, j);
    }
    std::shuffle(v.begin(), v.end(), rng);
    const std::vector<Entry> want = oracle(v, K);

    PoseTopK<K> one;
    one.clear();
    for (const Entry& e : v) one.insert(e.first, e.second);
    if (!same(one, want, "insert", n)) return false;

    // sixteen partial lists over interleaved subsets (4 lane groups x 4 waves), stored with a stride as the kernel's LDS
    // buffer is, then merged in order; and the same lists merged back to front
    constexpr int P = 16;
    std::vector<double> pc(P * K);
    std::vector<int32_t> pi(P * K);
    for (int p = 0; p < P; ++p) {
        PoseTopK<K> part;
        part.clear();
        for (int j = p; j < n; j += P) part.insert(v[j].first, v[j].second);
        for (int j = 0; j < K; ++j) {
            pc[j * P + p] = part.c[j];
            pi[j * P + p] = part.i[j];
        }
    }
    PoseTopK<K> fwd, bwd;
    fwd.clear();
    bwd.clear();
    for (int p = 0; p < P; ++p) fwd.merge(pc.data() + p, pi.data() + p, K, P);
    for (int p = P - 1; p >= 0; --p) bwd.merge(pc.data() + p, pi.data() + p, K, P);
    return same(fwd, want, "merge", n) && same(bwd, want, "merge (reversed)", n);
}

template <int K>
bool run_all(std::mt19937_64& rng) {
    for (int n : {0, 1, 2, 3, 15, 16, 17, 63, 64, 257, 2000})
        for (int levels : {0, 1, 3, 50})
            for (int rep = 0; rep < 4; ++rep)
                if (!run<K>(rng, n, levels)) return false;
    return true;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20240607);
    bool ok = run_all<1>(rng) && run_all<2>(rng) && run_all<4>(rng) && run_all<8>(rng) && run_all<16>(rng);
    for (int k = 1; k <= POSE_TOPK_MAX; ++k) ok = ok && pose_topk_size(k) >= k && pose_topk_size(k) < 2 * k + (k == 1);
    std::printf("pose_topk_host_check: %s\n", ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}
