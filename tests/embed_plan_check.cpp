// Stand-alone check of the embedding planner (hbk_embed_plan.h), run by
// tests/test_embed_plan.py as a child process built with -fsanitize=address,undefined.
// Arguments: graph files (written by the test). For every graph, precision and knob set
// of the case list it plans, asserts the plan's invariants and prints the plan as scalars
// and hashes; the test compares the output with the table recorded from the tree before
// the planner was split out of hbk_embed.hip, then the stack's one unit
// (tests/golden/embed_plan_parent.json).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hbk_embed_plan.h"

using namespace hbk;

namespace {

// ---- shared with the program that recorded the table: files, cases, printing ----

struct GraphFile {
  struct Op {
    int kind, kh, kw, cin, cout, act;
    float alpha;
    std::vector<float> w, b;
  };
  std::string name;
  int in_h = 0, in_w = 0;
  std::vector<int> starts;
  std::vector<Op> ops;
};

// int32: in_h, in_w, n_starts, n_ops; starts; per op: kind, kh, kw, cin, cout, act, n_w, n_b, f32 alpha, w, b
bool read_graph(const char* path, GraphFile& g) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  auto geti = [&](int& v) { return fread(&v, 4, 1, f) == 1; };
  int n_starts = 0, n_ops = 0;
  bool ok = geti(g.in_h) && geti(g.in_w) && geti(n_starts) && geti(n_ops) && n_starts >= 0 && n_starts <= 64 &&
            n_ops >= 0 && n_ops <= 256;
  g.starts.resize(ok ? n_starts : 0);
  for (int& s : g.starts) ok = ok && geti(s);
  for (int i = 0; ok && i < n_ops; ++i) {
    GraphFile::Op o{};
    int nw = 0, nb = 0;
    ok = geti(o.kind) && geti(o.kh) && geti(o.kw) && geti(o.cin) && geti(o.cout) && geti(o.act) && geti(nw) && geti(nb) &&
         fread(&o.alpha, 4, 1, f) == 1 && nw >= 0 && nb >= 0 && nw <= (1 << 24) && nb <= (1 << 16);
    if (!ok) break;
    o.w.resize(nw);
    o.b.resize(nb);
    ok = fread(o.w.data(), 4, nw, f) == size_t(nw) && fread(o.b.data(), 4, nb, f) == size_t(nb);
    g.ops.push_back(std::move(o));
  }
  fclose(f);
  const char* slash = strrchr(path, '/');
  g.name = slash ? slash + 1 : path;
  g.name = g.name.substr(0, g.name.find('.'));
  return ok;
}

struct KnobSet {
  const char* name;
  std::vector<std::pair<const char*, const char*>> env;
  bool se20_only;  // the pattern knobs touch no other graph
};

const std::vector<KnobSet>& knob_sets() {
  static const std::vector<KnobSet> sets = {
      {"default", {}, false},
      {"not3s", {{"HBK_EMBED_NO_T3S", "1"}}, true},
      {"p0", {{"HBK_EMBED_NO_P0S", "1"}, {"HBK_EMBED_NO_P1S", "1"}}, true},
      {"nodedup", {{"HBK_EMBED_NO_DEDUP", "1"}}, true},
      {"generic",
       {{"HBK_EMBED_NO_P0", "1"}, {"HBK_EMBED_NO_P1", "1"}, {"HBK_EMBED_NO_P2S", "1"}, {"HBK_EMBED_NO_T3S", "1"}},
       true},
      {"band5", {{"HBK_P0_BAND", "5"}}, true},
      {"band7", {{"HBK_P0_BAND", "7"}}, true},
      {"lds40", {{"HBK_EMBED_LDS_KB", "40"}}, false},
      {"lds156", {{"HBK_EMBED_LDS_KB", "156"}}, false},
      {"wlds", {{"HBK_EMBED_WEIGHTS", "lds"}}, false},
      {"wglobal", {{"HBK_EMBED_WEIGHTS", "global"}}, false},
  };
  return sets;
}

// The cases of one graph: every knob set in split precision; the default and nodedup in exact
// (the other knobs touch only the split-f16 layout and the pattern kernels). A graph whose
// name starts with "bad" is planned with the defaults only.
template <class F>
void for_each_case(const GraphFile& g, F&& run) {
  const bool se20 = g.name == "se20", bad = g.name.rfind("bad", 0) == 0;
  for (int split = 1; split >= 0; --split)
    for (const KnobSet& k : knob_sets()) {
      if (k.se20_only && !se20) continue;
      if (bad && k.env.size()) continue;
      if (!split && k.env.size() && strcmp(k.name, "nodedup")) continue;
      run(split != 0, k);
    }
}

uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

struct Out {  // a JSON array of numbers
  std::string s = "[";
  void i(long long v) { s += (s.size() > 1 ? "," : "") + std::to_string(v); }
  void f(double v) {
    char b[40];
    snprintf(b, sizeof(b), "%.17g", v);
    s += (s.size() > 1 ? "," : "") + std::string(b);
  }
  std::string done() { return s + "]"; }
};

// every scalar field of the argument structs (stages: the n_stages in use; the rest must be 0)
void put(Out& o, const ChainArgs& a) {
  for (long long v : {(long long)a.src_clip_stride, (long long)a.src_row_stride, (long long)a.ipc}) o.i(v);
  for (int k = 0; k < kMaxWin; ++k) o.i(a.row_off[k]);
  for (long long v : {(long long)a.C_src, (long long)a.in_ph, (long long)a.in_pw, (long long)a.W_in, (long long)a.out_ph,
                      (long long)a.out_pw, (long long)a.H_out, (long long)a.W_out, (long long)a.C_out,
                      (long long)a.out_img_stride, (long long)a.G, (long long)a.band, (long long)a.n_bands,
                      (long long)a.shrink, (long long)a.n_stages, (long long)a.wblob_floats, (long long)a.wstride,
                      (long long)a.lds_x, (long long)a.lds_y, (long long)a.lds_w, (long long)a.lds_k})
    o.i(v);
  for (int s = 0; s < a.n_stages; ++s) {
    const StageDesc& S = a.st[s];
    for (int v : {S.kh, S.kw, S.cin, S.cinp, S.cout, S.coutp, S.K, S.ksteps, S.act}) o.i(v);
    o.f(S.alpha);
    o.i(S.w_off);
    o.i(S.b_off);
  }
}
void put(Out& o, const XArgs& a) {
  for (long long v : {(long long)a.i2c_n, (long long)a.src_clip_stride, (long long)a.src_row_stride, (long long)a.ipc}) o.i(v);
  for (int k = 0; k < kMaxWin; ++k) o.i(a.row_off[k]);
  for (long long v : {(long long)a.C_src, (long long)a.cs0, (long long)a.im2col, (long long)a.in_ph, (long long)a.in_pw,
                      (long long)a.W_in, (long long)a.out_ph, (long long)a.out_pw, (long long)a.H_out, (long long)a.W_out,
                      (long long)a.C_out, (long long)a.out_img_stride, (long long)a.vec_out, (long long)a.raw_vec,
                      (long long)a.G, (long long)a.band, (long long)a.n_bands, (long long)a.shrink, (long long)a.n_stages,
                      (long long)a.w_halfs, (long long)a.b_floats, (long long)a.kt_n, (long long)a.lds_x,
                      (long long)a.lds_y, (long long)a.lds_w, (long long)a.lds_b, (long long)a.lds_k,
                      (long long)a.dbg_slot, (long long)a.dbg_skip})
    o.i(v);
  for (int s = 0; s < a.n_stages; ++s) {
    const XStage& S = a.st[s];
    for (int v : {S.kh, S.kw, S.cin, S.cout, S.coutr, S.cs_in, S.cs_out, S.ksteps, S.nblk, S.act}) o.i(v);
    o.f(S.alpha);
    for (int v : {S.w_off, S.w_lo, S.wrow, S.b_off, S.kt_off}) o.i(v);
  }
}
void put(Out& o, const P0Args& a) {
  for (int v : {a.H_in, a.H_out, a.n_bands}) o.i(v);
  o.f(a.alpha);
}
void put(Out& o, const P1Args& a) {
  for (int v : {a.H_in, a.H_out, a.n_bands}) o.i(v);
  o.f(a.alpha);
}
void put(Out& o, const P2sArgs& a) { o.f(a.alpha); }
void put(Out& o, const T3sArgs& a) {
  o.i(a.out_img_stride);
  o.f(a.alpha);
}

struct LaunchRow {
  std::string kernel;  // kind/n/flag
  std::string args;    // Out of the argument struct
  long long threads = 0, lds = 0, imgs_per_task = 0, n_bands = 0, below_2_31 = 0, min_src_stride = 0, out_stride_4 = 0;
  long long blob_bytes = 0, off[3] = {-1, -1, -1};  // where the 2nd .. 4th argument pointers point (-1: null)
  uint64_t hash = 0;
};

void print_launch(const char* key, const LaunchRow& r) {
  printf("\"%s\": {\"kernel\": \"%s\", \"args\": %s, \"launch\": [%lld,%lld,%lld,%lld,%lld,%lld,%lld], "
         "\"blob\": [%lld,%lld,%lld,%lld], \"hash\": \"%016llx\"}",
         key, r.kernel.c_str(), r.args.c_str(), r.threads, r.lds, r.imgs_per_task, r.n_bands, r.below_2_31,
         r.min_src_stride, r.out_stride_4, r.blob_bytes, r.off[0], r.off[1], r.off[2], (unsigned long long)r.hash);
}

void print_ints(const char* key, const std::vector<long long>& v) {
  printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? "," : "", v[i]);
  printf("]");
}

void print_case_head(bool first, const GraphFile& g, bool split, const KnobSet& k, int rc, const std::string& error) {
  std::string e;
  for (char c : error) e += (c == '"' || c == '\\') ? std::string("\\") + c : std::string(1, c);
  printf("%s\n{\"graph\": \"%s\", \"precision\": \"%s\", \"knobs\": \"%s\", \"rc\": %d, \"error\": \"%s\"",
         first ? "" : ",", g.name.c_str(), split ? "split" : "exact", k.name, rc, e.c_str());
}

// ---- end of the shared part ----

int g_failed = 0;
std::string g_where;
#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) {                                                                    \
      fprintf(stderr, "embed_plan_check: %s fails (%s)\n", #cond, g_where.c_str());   \
      ++g_failed;                                                                     \
    }                                                                                 \
  } while (0)

EmbedKnobs knobs_of(const KnobSet& k) {  // as read_embed_knobs reads them
  EmbedKnobs kn;
  for (const auto& [name, value] : k.env) {
    const std::string n = name;
    if (n == "HBK_EMBED_LDS_KB") kn.lds_kb_set = true, kn.lds_kb = atoi(value);
    else if (n == "HBK_EMBED_WEIGHTS") kn.weights = !strcmp(value, "lds") ? 1 : !strcmp(value, "global") ? 2 : 0;
    else if (n == "HBK_EMBED_NO_P0") kn.no_p0 = true;
    else if (n == "HBK_EMBED_NO_P0S") kn.no_p0s = true;
    else if (n == "HBK_EMBED_NO_P1") kn.no_p1 = true;
    else if (n == "HBK_EMBED_NO_P1S") kn.no_p1s = true;
    else if (n == "HBK_EMBED_NO_P2S") kn.no_p2s = true;
    else if (n == "HBK_EMBED_NO_T3S") kn.no_t3s = true;
    else if (n == "HBK_EMBED_NO_DEDUP") kn.no_dedup = true;
    else if (n == "HBK_P0_BAND") kn.p0_band = atoi(value);
    else CHECK(!"a knob of the case list");
  }
  return kn;
}

constexpr long long kCuLds = 160 * 1024;

void check_launch(const Launch& L, bool pattern) {
  CHECK(L.threads > 0 && L.threads % 64 == 0 && L.imgs_per_task >= 1 && L.n_bands >= 1);
  CHECK(L.lds_bytes > 0 && (long long)L.lds_bytes <= kCuLds);
  CHECK(!L.blob.empty() && L.name[0]);
  if (const XArgs* x = std::get_if<XArgs>(&L.args)) {
    // LDS regions (bytes): X, Y, weights (if resident), biases, group offsets
    const long long r[6] = {x->lds_x, x->lds_y, x->lds_w, x->lds_b, x->lds_k, (long long)L.lds_bytes};
    CHECK(r[0] == 0);
    for (int i = 0; i < 5; ++i) CHECK(r[i] % 16 == 0 && r[i] <= r[i + 1]);
    CHECK(r[3] - r[2] >= 2ll * x->w_halfs && r[4] - r[3] >= 4ll * x->b_floats && r[5] - r[4] >= 4ll * x->kt_n);
    CHECK((x->w_halfs == 0) == L.kernel.flag && x->G == L.imgs_per_task && x->n_bands == L.n_bands);
    CHECK(x->G >= 1 && x->band >= 1 && (long long)x->band * x->n_bands >= x->H_out);
    // the blob: weights, biases, group offsets, im2col taps
    const size_t* off = L.ptr_off;
    CHECK(off[0] == 0 && off[1] % 16 == 0 && off[2] % 16 == 0 && off[3] % 16 == 0);
    CHECK(off[1] <= off[2] && off[2] <= off[3] && off[3] + 4ull * x->i2c_n == L.blob.size());
    CHECK(off[1] + 4ull * x->b_floats <= off[2] && off[2] + 4ull * x->kt_n <= off[3]);
    CHECK(x->n_stages >= 1 && x->n_stages <= kMaxStages);
    for (int s = 0; s < kMaxStages; ++s) {
      const XStage& S = x->st[s];
      if (s >= x->n_stages) {
        static const XStage zero{};
        CHECK(!memcmp(&S, &zero, sizeof(S)));
        continue;
      }
      CHECK(S.w_off >= 0 && 2ull * (S.w_off + 2ll * S.w_lo) <= off[1] && S.w_lo == S.nblk * 32 * S.wrow);
      CHECK(S.b_off >= 0 && S.b_off + S.nblk * 32 <= x->b_floats);
      CHECK(S.kt_off >= 0 && S.kt_off + 2 * S.ksteps <= x->kt_n && S.wrow >= 16 * S.ksteps);
    }
    std::vector<int> kt(x->kt_n);
    memcpy(kt.data(), L.blob.data() + off[2], 4ull * x->kt_n);
    for (int v : kt) CHECK(v >= 0);
  } else if (const ChainArgs* a = std::get_if<ChainArgs>(&L.args)) {
    // LDS regions (floats): X, Y, weights (if resident), K offsets
    const long long r[5] = {a->lds_x, a->lds_y, a->lds_w, a->lds_k, (long long)L.lds_bytes / 4};
    CHECK(r[0] == 0 && L.lds_bytes % 16 == 0);
    for (int i = 0; i < 4; ++i) CHECK(r[i] % 4 == 0 && r[i] <= r[i + 1]);
    CHECK(L.kernel.flag ? r[3] == r[2] : r[3] - r[2] >= a->wblob_floats);
    CHECK(a->G == L.imgs_per_task && a->n_bands == L.n_bands && (long long)a->band * a->n_bands >= a->H_out);
    CHECK(L.blob.size() == 4ull * a->wblob_floats && a->n_stages >= 1 && a->n_stages <= kMaxStages);
    for (int s = 0; s < a->n_stages; ++s) {
      const StageDesc& S = a->st[s];
      CHECK(S.w_off >= 0 && S.w_off + 4ll * S.ksteps * a->wstride <= a->wblob_floats && S.cout <= a->wstride);
      CHECK(S.b_off >= 0 && S.b_off + L.kernel.n * 16 <= a->wblob_floats);
    }
  } else {
    CHECK(pattern && L.ptr_off[0] == 0 && L.ptr_off[1] % 16 == 0 && L.ptr_off[1] <= L.blob.size());
  }
  CHECK(pattern == (L.kernel.kind != Kern::exact && L.kernel.kind != Kern::x3));
}

void check_program(const ProgramPlan& prog, const EmbedHostPlan& p, bool clip) {
  CHECK(!prog.chains.empty());
  for (size_t k = 0; k < prog.chains.size(); ++k) {
    const ChainHost& c = prog.chains[k];
    check_launch(c.base, false);
    if (c.pattern) check_launch(*c.pattern, true);
    CHECK(!c.pattern || p.split_f16);
    CHECK(p.split_f16 == std::holds_alternative<XArgs>(c.base.args));
    CHECK((c.src_buf == -1) == (k == 0) && c.src_buf <= 1 && c.dst_buf >= -1 && c.dst_buf <= 1);
    CHECK(c.src_buf < 0 || c.src_buf != c.dst_buf);
    CHECK(c.imgs_per_unit >= 1 && c.out_img_stride >= 1 && c.macs_per_img > 0);
    if (c.dst_buf >= 0) CHECK(prog.buf_floats[c.dst_buf] >= c.out_img_stride * c.imgs_per_unit);  // the buffer holds it
    if (k + 1 < prog.chains.size()) CHECK(c.dst_buf >= 0 && prog.chains[k + 1].src_buf == c.dst_buf);
  }
  const ChainHost& last = prog.chains.back();
  if (prog.gather_buf >= 0) {
    CHECK(clip && last.dst_buf == prog.gather_buf && int(prog.gather_src.size()) == p.n_win && prog.n_src >= 1);
    for (int i : prog.gather_src) CHECK(i >= 0 && i < prog.n_src);
    CHECK(last.out_img_stride * last.imgs_per_unit == int64_t(prog.n_src) * p.out_dim);
  } else {
    CHECK(last.dst_buf == -1 && prog.gather_src.empty());
    CHECK(last.out_img_stride * last.imgs_per_unit == int64_t(clip ? p.n_win : 1) * p.out_dim);
  }
}

const char* kind_name(Kern k) {
  switch (k) {
    case Kern::exact: return "exact";
    case Kern::x3: return "x3";
    case Kern::p0_band: return "p0";
    case Kern::p0s: return "p0s";
    case Kern::p1: return "p1";
    case Kern::p1s: return "p1s";
    case Kern::p2s: return "p2s";
    case Kern::t3s: return "t3s";
  }
  return "?";
}

LaunchRow row_of(const Launch& L) {
  LaunchRow r;
  r.kernel = std::string(kind_name(L.kernel.kind)) + "/" + std::to_string(L.kernel.n) + "/" + (L.kernel.flag ? "1" : "0");
  Out o;
  std::visit([&](const auto& a) { put(o, a); }, L.args);
  r.args = o.done();
  r.threads = L.threads;
  r.lds = (long long)L.lds_bytes;
  r.imgs_per_task = L.imgs_per_task;
  r.n_bands = L.n_bands;
  r.below_2_31 = L.tasks_below_2_31;
  r.min_src_stride = L.min_src_stride;
  r.out_stride_4 = L.out_stride_4;
  r.blob_bytes = (long long)L.blob.size();
  const int n_ptr = std::holds_alternative<XArgs>(L.args) ? 4 : std::holds_alternative<ChainArgs>(L.args) ? 1 : 2;
  for (int i = 1; i < n_ptr; ++i)
    if (n_ptr == 4 || L.ptr_off[i] < L.blob.size()) r.off[i - 1] = (long long)L.ptr_off[i];
  r.hash = fnv1a(L.blob.data(), L.blob.size());
  return r;
}

void print_program(const char* key, const ProgramPlan& prog) {
  printf(",\n \"%s\": {", key);
  print_ints("buf_floats", {prog.buf_floats[0], prog.buf_floats[1]});
  std::vector<long long> gth = {prog.gather_buf, prog.n_src};
  gth.insert(gth.end(), prog.gather_src.begin(), prog.gather_src.end());
  printf(", ");
  print_ints("gather", gth);
  printf(", \"chains\": [");
  for (size_t k = 0; k < prog.chains.size(); ++k) {
    const ChainHost& c = prog.chains[k];
    printf("%s\n  {", k ? "," : "");
    print_ints("io", {c.src_buf, c.dst_buf, c.out_floats, c.imgs_per_unit});
    printf(", \"macs\": %.17g, ", c.macs_per_img);
    print_launch("base", row_of(c.base));
    if (c.pattern) {
      printf(", ");
      print_launch("pattern", row_of(*c.pattern));
    }
    printf("}");
  }
  printf("]}");
}

}  // namespace

int main(int argc, char** argv) {
  printf("{\"cases\": [");
  bool first = true;
  for (int i = 1; i < argc; ++i) {
    GraphFile g;
    if (!read_graph(argv[i], g)) {
      fprintf(stderr, "embed_plan_check: cannot read %s\n", argv[i]);
      return 1;
    }
    std::vector<OpIn> ops;
    for (const GraphFile::Op& o : g.ops)
      ops.push_back(OpIn{o.kind, o.kh, o.kw, o.cin, o.cout, o.act, o.alpha, o.w.empty() ? nullptr : o.w.data(),
                         o.b.empty() ? nullptr : o.b.data()});
    for_each_case(g, [&](bool split, const KnobSet& k) {
      g_where = g.name + (split ? " split " : " exact ") + k.name;
      EmbedHostPlan p;
      const int rc = plan_embed(ops, g.in_h, g.in_w, g.starts, split, knobs_of(k), p);
      print_case_head(first, g, split, k, rc, p.error);
      first = false;
      CHECK((rc == kPlanOk) == p.error.empty());
      if (rc == kPlanOk) {
        CHECK(p.n_prefix >= 1 && p.n_prefix < int(ops.size()) && p.split_stride >= 1 && p.seq_frames >= g.in_h);
        check_program(p.clip, p, true);
        check_program(p.win, p, false);
        printf(",\n ");
        print_ints("plan", {p.n_prefix, p.split_stride, p.seq_frames, p.out_dim});
        printf(", \"macs\": [%.17g,%.17g]", p.prefix_macs, p.tail_macs);
        print_program("clip", p.clip);
        print_program("win", p.win);
      }
      printf("}");
    });
  }
  printf("\n]}\n");
  return g_failed ? 1 : 0;
}
