// Native text-format parsers for the data loader (CPU, multi-threaded).
// Reference: common/dataloader (HdfsDataSet record iteration) + the per-app
// parsers (NMFETDataParser.java:39, MLR/GBT/Lasso libsvm-style rows, LDA
// word lists). Python line-splitting is ~50x slower on the multi-GB inputs
// the reference targets; this scans the raw bytes of a split once per
// thread and emits torch tensors directly.

#include <torch/extension.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace {

struct Cursor {
  const char* p;
  const char* end;

  bool done() const { return p >= end; }
  void skip_ws_inline() {
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\r')) ++p;
  }
  void next_line() {
    while (p < end && *p != '\n') ++p;
    if (p < end) ++p;
  }
  bool at_comment_or_empty() {
    skip_ws_inline();
    return p >= end || *p == '#' || *p == '\n';
  }
  long read_long() {
    skip_ws_inline();
    char* q;
    long v = strtol(p, &q, 10);
    p = (q == p && p < end) ? p + 1 : q;   // always progress on garbage
    return v;
  }
  double read_double() {
    skip_ws_inline();
    char* q;
    double v = strtod(p, &q);
    p = (q == p && p < end) ? p + 1 : q;
    return v;
  }
  bool eol() {
    skip_ws_inline();
    return p >= end || *p == '\n';
  }
};

// split [start,end) into n chunks aligned to line starts
std::vector<std::pair<const char*, const char*>> line_chunks(
    const char* base, int64_t len, int n) {
  std::vector<std::pair<const char*, const char*>> out;
  std::vector<const char*> bounds(n + 1);
  bounds[0] = base;
  bounds[n] = base + len;
  for (int i = 1; i < n; ++i) {
    const char* p = base + (len * i) / n;
    while (p < base + len && *p != '\n') ++p;
    if (p < base + len) ++p;
    bounds[i] = p;
  }
  for (int i = 0; i < n; ++i)
    out.emplace_back(bounds[i], std::max(bounds[i], bounds[i + 1]));
  return out;
}

int nthreads() {
  // HARMONY_PARSE_THREADS caps the per-process scan threads: with W
  // loader processes per node (one per GPU), W * hw threads oversubscribe
  // the cores 8x and parsing runs 5x SLOWER than linear (measured in
  // scripts/ingest_bench.py) — the loader sets it to cores/world.
  if (const char* e = std::getenv("HARMONY_PARSE_THREADS")) {
    int v = std::atoi(e);
    if (v > 0) return std::min(v, 64);
  }
  unsigned hw = std::thread::hardware_concurrency();
  return std::max(1u, std::min(hw, 16u));
}

}  // namespace

// "rowId: col,val col,val ..." -> (rows, cols, vals)
std::vector<torch::Tensor> parse_nmf_bytes(const std::string& buf) {
  const int T = nthreads();
  auto chunks = line_chunks(buf.data(), (int64_t)buf.size(), T);
  std::vector<std::vector<int64_t>> rows(T), cols(T);
  std::vector<std::vector<float>> vals(T);
  std::vector<std::thread> ths;
  for (int t = 0; t < T; ++t) {
    ths.emplace_back([&, t] {
      Cursor c{chunks[t].first, chunks[t].second};
      while (!c.done()) {
        if (c.at_comment_or_empty()) { c.next_line(); continue; }
        long r = c.read_long();
        c.skip_ws_inline();
        if (c.p < c.end && *c.p == ':') ++c.p;
        while (!c.eol()) {
          long col = c.read_long();
          c.skip_ws_inline();
          if (c.p < c.end && *c.p == ',') ++c.p;
          double v = c.read_double();
          rows[t].push_back(r);
          cols[t].push_back(col);
          vals[t].push_back((float)v);
        }
        c.next_line();
      }
    });
  }
  for (auto& th : ths) th.join();
  int64_t total = 0;
  for (auto& v : rows) total += (int64_t)v.size();
  auto ro = torch::empty({total}, torch::kInt64);
  auto co = torch::empty({total}, torch::kInt64);
  auto vo = torch::empty({total}, torch::kFloat32);
  int64_t off = 0;
  for (int t = 0; t < T; ++t) {
    int64_t n = (int64_t)rows[t].size();
    if (n) {
      std::memcpy(ro.data_ptr<int64_t>() + off, rows[t].data(), n * 8);
      std::memcpy(co.data_ptr<int64_t>() + off, cols[t].data(), n * 8);
      std::memcpy(vo.data_ptr<float>() + off, vals[t].data(), n * 4);
    }
    off += n;
  }
  return {ro, co, vo};
}

// "label idx:val idx:val ..." -> (X dense [n,F], y [n])
std::vector<torch::Tensor> parse_libsvm_bytes(const std::string& buf,
                                              int64_t num_features) {
  const int T = nthreads();
  auto chunks = line_chunks(buf.data(), (int64_t)buf.size(), T);
  std::vector<std::vector<float>> Xs(T);
  std::vector<std::vector<float>> ys(T);
  std::vector<std::thread> ths;
  for (int t = 0; t < T; ++t) {
    ths.emplace_back([&, t] {
      Cursor c{chunks[t].first, chunks[t].second};
      while (!c.done()) {
        if (c.at_comment_or_empty()) { c.next_line(); continue; }
        double lab = c.read_double();
        size_t base = Xs[t].size();
        Xs[t].resize(base + num_features, 0.f);
        while (!c.eol()) {
          long idx = c.read_long();
          c.skip_ws_inline();
          if (c.p < c.end && *c.p == ':') ++c.p;
          double v = c.read_double();
          if (idx >= 0 && idx < num_features) Xs[t][base + idx] = (float)v;
        }
        ys[t].push_back((float)lab);
        c.next_line();
      }
    });
  }
  for (auto& th : ths) th.join();
  int64_t total = 0;
  for (auto& v : ys) total += (int64_t)v.size();
  auto X = torch::empty({total, num_features}, torch::kFloat32);
  auto y = torch::empty({total}, torch::kFloat32);
  int64_t off = 0;
  for (int t = 0; t < T; ++t) {
    int64_t n = (int64_t)ys[t].size();
    if (n) {
      std::memcpy(X.data_ptr<float>() + off * num_features, Xs[t].data(),
                  n * num_features * 4);
      std::memcpy(y.data_ptr<float>() + off, ys[t].data(), n * 4);
    }
    off += n;
  }
  return {X, y};
}

// "label idx:val idx:val ..." -> CSR (row_ptr int64 [n+1], col int32 [nnz],
// val float32 [nnz], y float32 [n]). Same row rules as parse_libsvm_bytes
// (indices outside [0, num_features) dropped, a repeated index keeps its
// last value) but neither time nor memory depends on num_features: entries
// stay in file order, and a repeated index keeps the position of its first
// occurrence with the value of its last, so each (row, col) appears once.
std::vector<torch::Tensor> parse_libsvm_csr_bytes(const std::string& buf,
                                                  int64_t num_features) {
  TORCH_CHECK(num_features >= 0 && num_features < ((int64_t)1 << 31),
              "num_features must be below 2^31");
  const int T = nthreads();
  auto chunks = line_chunks(buf.data(), (int64_t)buf.size(), T);
  std::vector<std::vector<int32_t>> cols(T);
  std::vector<std::vector<float>> vals(T), ys(T);
  std::vector<std::vector<int64_t>> lens(T);
  std::vector<std::thread> ths;
  for (int t = 0; t < T; ++t) {
    ths.emplace_back([&, t] {
      Cursor c{chunks[t].first, chunks[t].second};
      auto& cs = cols[t];
      auto& vs = vals[t];
      std::vector<std::pair<int32_t, int64_t>> order;   // (col, position)
      while (!c.done()) {
        if (c.at_comment_or_empty()) { c.next_line(); continue; }
        double lab = c.read_double();
        const size_t base = cs.size();
        bool ascending = true;
        while (!c.eol()) {
          long idx = c.read_long();
          c.skip_ws_inline();
          if (c.p < c.end && *c.p == ':') ++c.p;
          double v = c.read_double();
          if (idx < 0 || idx >= num_features) continue;
          if (cs.size() > base && (int32_t)idx <= cs.back())
            ascending = false;
          cs.push_back((int32_t)idx);
          vs.push_back((float)v);
        }
        if (!ascending) {
          // only an unsorted row can repeat an index: sort (col, position)
          // pairs, move each run's last value to its first position and
          // drop the rest
          order.clear();
          for (size_t i = base; i < cs.size(); ++i)
            order.emplace_back(cs[i], (int64_t)i);
          std::sort(order.begin(), order.end());
          bool dup = false;
          for (size_t i = 0; i < order.size();) {
            size_t j = i + 1;
            while (j < order.size() && order[j].first == order[i].first) ++j;
            if (j > i + 1) {
              dup = true;
              vs[order[i].second] = vs[order[j - 1].second];
              for (size_t k = i + 1; k < j; ++k) cs[order[k].second] = -1;
            }
            i = j;
          }
          if (dup) {
            size_t w = base;
            for (size_t i = base; i < cs.size(); ++i)
              if (cs[i] >= 0) { cs[w] = cs[i]; vs[w] = vs[i]; ++w; }
            cs.resize(w);
            vs.resize(w);
          }
        }
        lens[t].push_back((int64_t)(cs.size() - base));
        ys[t].push_back((float)lab);
        c.next_line();
      }
    });
  }
  for (auto& th : ths) th.join();
  int64_t n = 0, nnz = 0;
  for (int t = 0; t < T; ++t) {
    n += (int64_t)ys[t].size();
    nnz += (int64_t)cols[t].size();
  }
  auto rp = torch::empty({n + 1}, torch::kInt64);
  auto co = torch::empty({nnz}, torch::kInt32);
  auto vo = torch::empty({nnz}, torch::kFloat32);
  auto y = torch::empty({n}, torch::kFloat32);
  auto* rpp = rp.data_ptr<int64_t>();
  rpp[0] = 0;
  int64_t r = 0, off = 0;
  for (int t = 0; t < T; ++t) {
    const int64_t m = (int64_t)cols[t].size();
    if (m) {
      std::memcpy(co.data_ptr<int32_t>() + off, cols[t].data(), m * 4);
      std::memcpy(vo.data_ptr<float>() + off, vals[t].data(), m * 4);
    }
    off += m;
    if (!ys[t].empty())
      std::memcpy(y.data_ptr<float>() + r, ys[t].data(), ys[t].size() * 4);
    for (int64_t L : lens[t]) {
      rpp[r + 1] = rpp[r] + L;
      ++r;
    }
  }
  return {rp, co, vo, y};
}

// "word word word ..." one doc per line -> (doc_offsets [n+1], words)
std::vector<torch::Tensor> parse_lda_bytes(const std::string& buf) {
  const int T = nthreads();
  auto chunks = line_chunks(buf.data(), (int64_t)buf.size(), T);
  std::vector<std::vector<int64_t>> words(T), lens(T);
  std::vector<std::thread> ths;
  for (int t = 0; t < T; ++t) {
    ths.emplace_back([&, t] {
      Cursor c{chunks[t].first, chunks[t].second};
      while (!c.done()) {
        if (c.at_comment_or_empty()) { c.next_line(); continue; }
        int64_t n = 0;
        while (!c.eol()) {
          words[t].push_back(c.read_long());
          ++n;
        }
        lens[t].push_back(n);
        c.next_line();
      }
    });
  }
  for (auto& th : ths) th.join();
  int64_t ndocs = 0, nwords = 0;
  for (int t = 0; t < T; ++t) {
    ndocs += (int64_t)lens[t].size();
    nwords += (int64_t)words[t].size();
  }
  auto off = torch::empty({ndocs + 1}, torch::kInt64);
  auto wo = torch::empty({nwords}, torch::kInt64);
  int64_t d = 0, w = 0;
  auto* op = off.data_ptr<int64_t>();
  op[0] = 0;
  for (int t = 0; t < T; ++t) {
    if (!words[t].empty())
      std::memcpy(wo.data_ptr<int64_t>() + w, words[t].data(),
                  words[t].size() * 8);
    w += (int64_t)words[t].size();
    for (int64_t L : lens[t]) {
      op[d + 1] = op[d] + L;
      ++d;
    }
  }
  return {off, wo};
}

// Pregel adjacency lists (reference DefaultGraphParser.java:44 and
// NoneEdgeValueGraphParser.java:48): unweighted "src dst dst ..." or
// weighted "src dst w dst w ..." with integer weights (a trailing unpaired
// token is ignored, as upstream does). A line holding only "src" is a
// vertex without out-edges: it emits no edge but still counts towards
// max_id. -> (src [E], dst [E], w float32 [E] (empty if unweighted),
// max_id [1], -1 when the input names no vertex)
std::vector<torch::Tensor> parse_graph_bytes(const std::string& buf,
                                             bool weighted) {
  const int T = nthreads();
  auto chunks = line_chunks(buf.data(), (int64_t)buf.size(), T);
  std::vector<std::vector<int64_t>> srcs(T), dsts(T);
  std::vector<std::vector<float>> ws(T);
  std::vector<int64_t> maxid(T, -1);
  std::vector<std::thread> ths;
  for (int t = 0; t < T; ++t) {
    ths.emplace_back([&, t] {
      Cursor c{chunks[t].first, chunks[t].second};
      int64_t mx = -1;
      while (!c.done()) {
        if (c.at_comment_or_empty()) { c.next_line(); continue; }
        const int64_t s = c.read_long();
        mx = std::max(mx, s);
        while (!c.eol()) {
          const int64_t d = c.read_long();
          float w = 0.f;
          if (weighted) {
            if (c.eol()) break;            // unpaired trailing token
            w = (float)c.read_long();
          }
          srcs[t].push_back(s);
          dsts[t].push_back(d);
          if (weighted) ws[t].push_back(w);
          mx = std::max(mx, d);
        }
        c.next_line();
      }
      maxid[t] = mx;
    });
  }
  for (auto& th : ths) th.join();
  int64_t total = 0, mx = -1;
  for (int t = 0; t < T; ++t) {
    total += (int64_t)srcs[t].size();
    mx = std::max(mx, maxid[t]);
  }
  auto so = torch::empty({total}, torch::kInt64);
  auto dn = torch::empty({total}, torch::kInt64);
  auto wo = torch::empty({weighted ? total : 0}, torch::kFloat32);
  int64_t off = 0;
  for (int t = 0; t < T; ++t) {
    int64_t n = (int64_t)srcs[t].size();
    if (n) {
      std::memcpy(so.data_ptr<int64_t>() + off, srcs[t].data(), n * 8);
      std::memcpy(dn.data_ptr<int64_t>() + off, dsts[t].data(), n * 8);
      if (weighted)
        std::memcpy(wo.data_ptr<float>() + off, ws[t].data(), n * 4);
    }
    off += n;
  }
  auto mo = torch::empty({1}, torch::kInt64);
  mo.data_ptr<int64_t>()[0] = mx;
  return {so, dn, wo, mo};
}
