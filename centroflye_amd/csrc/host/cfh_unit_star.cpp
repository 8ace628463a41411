// cfh_unit_star.cpp — the de Bruijn purification and the re-phasing of stage 4 (include/cfhost.h: cfh_unit_star).
// Plain C++17; no GPU code here.
//
// Reference behaviour restated (never copied) from scripts/better_consensus_unit_reconstruction.py:
//   :20-36   DeBruijnGraph / add_kmer(s)   a networkx MultiDiGraph, one edge per k-mer (k-1)-mer -> (k-1)-mer
//   :38-51   remove_tips
//   :53-81   collapse_nonbranching_paths
//   :83-119  purify_graph
//   :122-126 get_coverage                  min of the edge's coverage list
//   :170-190 get_polished_unit             smallest edge tuple, minus k-1 bases; edlib HW re-phasing
// The output depends on the MultiDiGraph's bookkeeping, which is emulated here: nodes keep their insertion order (a
// removed node that comes back goes to the end), a new edge of a (u, v) pair gets the key len(keys of the pair), raised
// while taken (networkx MultiGraph.new_edge_key), and an edge tuple (u, v, key) orders by the node strings, then the key.
// Only the minimum of an edge's coverage list is ever read, so that is all an edge keeps.
#include "cfhost.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <new>
#include <set>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace {

struct UsError {
    int code;
    std::string msg;
};

struct Node {
    std::string name;
    bool alive = true;
    int in = 0, out = 0;                   // degrees; a self-loop counts once in each
    std::vector<int> edges;                // incident edge ids (dead ones are dropped lazily)
};

struct Edge {
    int u, v;
    int64_t key;
    std::string kmer;
    int64_t cov;
    bool alive = true;
};

struct Graph {
    int k;
    std::vector<Node> nodes;               // in insertion order; dead entries stay
    std::vector<Edge> edges;
    std::unordered_map<std::string, int> live;    // name -> live node id
    std::map<std::pair<int, int>, std::set<int64_t>> keys;   // (u, v) -> keys in use
    int64_t n_nodes = 0, n_edges = 0;

    int node(const std::string& s) {
        auto it = live.find(s);
        if (it != live.end()) return it->second;
        nodes.emplace_back();
        nodes.back().name = s;
        ++n_nodes;
        return live[s] = (int)nodes.size() - 1;
    }
    // add_edge(u, v, key=key_or_auto, edge_kmer=, coverages=): an explicit key that is taken overwrites that edge's data
    // (u and v by value: node() may grow `nodes`, and a caller may pass a name that lives there)
    void add_edge(const std::string us, const std::string vs, int64_t key, bool auto_key, const std::string& kmer, int64_t cov) {
        const int u = node(us), v = node(vs);
        auto& ks = keys[{u, v}];
        if (auto_key) {
            key = (int64_t)ks.size();
            while (ks.count(key)) ++key;
        } else if (ks.count(key)) {
            for (int e : nodes[(size_t)u].edges) {
                Edge& x = edges[(size_t)e];
                if (x.alive && x.u == u && x.v == v && x.key == key) { x.kmer = kmer; x.cov = cov; return; }
            }
        }
        ks.insert(key);
        edges.push_back(Edge{u, v, key, kmer, cov});
        const int id = (int)edges.size() - 1;
        nodes[(size_t)u].edges.push_back(id);
        if (v != u) nodes[(size_t)v].edges.push_back(id);
        ++nodes[(size_t)u].out;
        ++nodes[(size_t)v].in;
        ++n_edges;
    }
    void remove_edge(int e) {
        Edge& x = edges[(size_t)e];
        x.alive = false;
        auto it = keys.find({x.u, x.v});
        it->second.erase(x.key);
        if (it->second.empty()) keys.erase(it);
        --nodes[(size_t)x.u].out;
        --nodes[(size_t)x.v].in;
        --n_edges;
    }
    void remove_node(int n) {
        for (int e : nodes[(size_t)n].edges)
            if (edges[(size_t)e].alive) remove_edge(e);
        nodes[(size_t)n].alive = false;
        nodes[(size_t)n].edges.clear();
        live.erase(nodes[(size_t)n].name);
        --n_nodes;
    }
    std::vector<int> live_nodes() const {
        std::vector<int> r;
        for (int i = 0; i < (int)nodes.size(); ++i)
            if (nodes[(size_t)i].alive) r.push_back(i);
        return r;
    }
    std::vector<int> live_edges() const {
        std::vector<int> r;
        for (int i = 0; i < (int)edges.size(); ++i)
            if (edges[(size_t)i].alive) r.push_back(i);
        return r;
    }
    // the one live edge into (in = true) or out of n
    int only_edge(int n, bool in) const {
        for (int e : nodes[(size_t)n].edges) {
            const Edge& x = edges[(size_t)e];
            if (x.alive && (in ? x.v : x.u) == n) return e;
        }
        return -1;
    }
    bool tuple_less(int a, int b) const {     // (u, v, key) as Python compares the tuples
        const Edge &x = edges[(size_t)a], &y = edges[(size_t)b];
        int c = nodes[(size_t)x.u].name.compare(nodes[(size_t)y.u].name);
        if (c) return c < 0;
        c = nodes[(size_t)x.v].name.compare(nodes[(size_t)y.v].name);
        if (c) return c < 0;
        return x.key < y.key;
    }

    void collapse() {                          // :53-81 (every edge has the same colour)
        for (int n : live_nodes()) {
            if (!nodes[(size_t)n].alive || n_nodes <= 1 || nodes[(size_t)n].in != 1 || nodes[(size_t)n].out != 1) continue;
            const int ei = only_edge(n, true), eo = only_edge(n, false);
            const Edge in_e = edges[(size_t)ei], out_e = edges[(size_t)eo];
            const std::string kmer = in_e.kmer + out_e.kmer.substr((size_t)(k - 1));
            add_edge(nodes[(size_t)in_e.u].name, nodes[(size_t)out_e.v].name, 0, true, kmer, std::min(in_e.cov, out_e.cov));
            remove_node(n);
        }
    }
    void remove_tips() {                       // :38-51
        for (;;) {
            std::vector<int> del;
            for (int n : live_nodes()) {
                const Node& x = nodes[(size_t)n];
                if (x.in == 0 && x.out == 0) continue;
                if (x.in == 0 || x.out == 0) del.push_back(n);
            }
            if (del.empty()) return;
            for (int n : del) remove_node(n);
        }
    }
    void remove_isolates() {
        for (int n : live_nodes())
            if (nodes[(size_t)n].in == 0 && nodes[(size_t)n].out == 0) remove_node(n);
    }
    // Weakly connected?  (networkx raises on the null graph; the caller decides what that means.)
    bool connected() const {
        std::vector<int> ln = live_nodes();
        if (ln.empty()) return false;
        std::vector<char> seen(nodes.size(), 0);
        std::vector<int> st{ln[0]};
        seen[(size_t)ln[0]] = 1;
        int64_t reached = 1;
        while (!st.empty()) {
            const int n = st.back();
            st.pop_back();
            for (int e : nodes[(size_t)n].edges) {
                const Edge& x = edges[(size_t)e];
                if (!x.alive) continue;
                const int o = x.u == n ? x.v : x.u;
                if (!seen[(size_t)o]) { seen[(size_t)o] = 1; ++reached; st.push_back(o); }
            }
        }
        return reached == n_nodes;
    }
    // Bridges of the undirected multigraph (iterative Tarjan over edge ids: a parallel edge or a self-loop is never a bridge).
    std::vector<char> bridges() const {
        std::vector<char> is_bridge(edges.size(), 0);
        std::vector<int> tin(nodes.size(), -1), low(nodes.size(), 0);
        struct Frame { int n, via, pos; };
        int timer = 0;
        for (int root : live_nodes()) {
            if (tin[(size_t)root] >= 0) continue;
            std::vector<Frame> st{{root, -1, 0}};
            tin[(size_t)root] = low[(size_t)root] = timer++;
            while (!st.empty()) {
                Frame& f = st.back();
                const Node& x = nodes[(size_t)f.n];
                if (f.pos < (int)x.edges.size()) {
                    const int e = x.edges[(size_t)f.pos++];
                    const Edge& y = edges[(size_t)e];
                    if (!y.alive || e == f.via || y.u == y.v) continue;
                    const int o = y.u == f.n ? y.v : y.u;
                    if (tin[(size_t)o] >= 0) {
                        low[(size_t)f.n] = std::min(low[(size_t)f.n], tin[(size_t)o]);
                    } else {
                        tin[(size_t)o] = low[(size_t)o] = timer++;
                        st.push_back({o, e, 0});
                    }
                } else {
                    const Frame done = f;
                    st.pop_back();
                    if (!st.empty()) {
                        const int p = st.back().n;
                        low[(size_t)p] = std::min(low[(size_t)p], low[(size_t)done.n]);
                        if (low[(size_t)done.n] > tin[(size_t)p]) is_bridge[(size_t)done.via] = 1;
                    }
                }
            }
        }
        return is_bridge;
    }

    void purify(int64_t* n_removed) {         // :83-119
        std::vector<int> le = live_edges();
        int first = -1;
        for (int e : le) {
            const Edge& x = edges[(size_t)e];
            if (nodes[(size_t)x.u].out != 1 || nodes[(size_t)x.v].in != 1) continue;
            if (first < 0 || x.cov > edges[(size_t)first].cov || (x.cov == edges[(size_t)first].cov && tuple_less(e, first))) first = e;
        }
        if (first < 0) throw UsError{-61, "purify_graph: no edge has a tail of out-degree 1 and a head of in-degree 1 (the reference fails on graph.edges[None])"};
        const Edge fe = edges[(size_t)first];
        const std::string fu = nodes[(size_t)fe.u].name, fv = nodes[(size_t)fe.v].name;
        remove_edge(first);
        *n_removed = 0;
        for (;;) {
            // the first edge in (coverage, edge tuple) order whose removal leaves the graph weakly connected: a non-bridge of a
            // connected graph (removing an edge never connects a disconnected one)
            le = live_edges();
            if (le.empty() || !connected()) break;
            const std::vector<char> br = bridges();
            int best = -1;
            for (int e : le) {
                if (br[(size_t)e]) continue;
                if (best < 0 || edges[(size_t)e].cov < edges[(size_t)best].cov ||
                    (edges[(size_t)e].cov == edges[(size_t)best].cov && tuple_less(e, best))) best = e;
            }
            if (best < 0) break;
            remove_edge(best);
            ++*n_removed;
            remove_isolates();
            if (n_nodes == 0) throw UsError{-62, "purify_graph: the graph became empty (the reference fails: connectivity of the null graph)"};
            if (!connected()) throw UsError{-63, "purify_graph: the graph is no longer weakly connected (the reference fails an assertion)"};
            collapse();
        }
        add_edge(fu, fv, fe.key, false, fe.kmer, fe.cov);
        remove_tips();
        collapse();
    }
};

// ---- edlib-compatible HW alignment (locations[0] of edlib.align(query, target, mode='HW', task='locations')) ----
// Bit-parallel edit distance (Myers 1999) over 64-row blocks with horizontal carries between blocks (Hyyro 2003), all
// blocks in every column; last_row[j] = D[m][j], the cost of the query against the best target substring ending at j.
// hin_top is the horizontal delta entering the top row: 0 for HW (free start), +1 for SHW (the target starts at 0).
typedef uint64_t Word;

static void last_row(const std::string& q, const std::string& t, int hin_top, std::vector<int>& row) {
    const int m = (int)q.size(), n = (int)t.size(), B = (m + 63) / 64;
    std::vector<Word> peq((size_t)256 * B, 0);
    for (int i = 0; i < m; ++i) peq[(size_t)(unsigned char)q[(size_t)i] * B + i / 64] |= Word(1) << (i % 64);
    std::vector<Word> P((size_t)B, ~Word(0)), M((size_t)B, 0);
    const int tb = (m - 1) / 64, tbit = (m - 1) % 64;
    int score = m;                             // D[m][-1]
    row.assign((size_t)n, 0);
    for (int j = 0; j < n; ++j) {
        const Word* eqc = peq.data() + (size_t)(unsigned char)t[(size_t)j] * B;
        int h = hin_top;
        for (int b = 0; b < B; ++b) {
            Word eq = eqc[b];
            const Word pv = P[(size_t)b], mv = M[(size_t)b];
            const Word xv = eq | mv;
            if (h < 0) eq |= 1;
            const Word xh = (((eq & pv) + pv) ^ pv) | eq;
            Word ph = mv | ~(xh | pv), mh = pv & xh;
            if (b == tb) score += (int)((ph >> tbit) & 1) - (int)((mh >> tbit) & 1);
            const int hout = (int)(ph >> 63) - (int)(mh >> 63);
            ph <<= 1;
            mh <<= 1;
            if (h < 0) mh |= 1;
            else if (h > 0) ph |= 1;
            P[(size_t)b] = mh | ~(xv | ph);
            M[(size_t)b] = ph & xv;
            h = hout;
        }
        row[(size_t)j] = score;
    }
}

// The positions edlib reports: every p with D[m][p] == min, ascending, where p = -1 (query before the target, cost m) is a
// candidate only when m is not a multiple of 64 (edlib reads it off the padded rows of its last block).
static std::vector<int> best_positions(const std::vector<int>& row, int m, int* best) {
    const bool minus1 = m % 64 != 0;
    int b = minus1 ? m : (row.empty() ? m : row[0]);
    for (int v : row) b = std::min(b, v);
    std::vector<int> pos;
    if (minus1 && b == m) pos.push_back(-1);
    for (int j = 0; j < (int)row.size(); ++j)
        if (row[(size_t)j] == b) pos.push_back(j);
    *best = b;
    return pos;
}

// (start, end) of edlib's first location; the start comes from the SHW alignment of the reversed query against the
// reversed target prefix [0, end], whose LAST best position edlib takes (the alignment that covers the most target).
static void hw_first_location(const std::string& q, const std::string& t, int* dist, int* start, int* end) {
    std::vector<int> row;
    last_row(q, t, 0, row);
    const std::vector<int> ends = best_positions(row, (int)q.size(), dist);
    *end = ends[0];
    if (*end < 0) { *start = 0; return; }
    const std::string rq(q.rbegin(), q.rend());
    const std::string rt(t.rend() - (*end + 1), t.rend());
    last_row(rq, rt, 1, row);
    int best_shw = 0;
    const std::vector<int> sp = best_positions(row, (int)q.size(), &best_shw);
    *start = *end - sp.back();
}

static int unit_star(int32_t k, const char* kmers, const int64_t* counts, int64_t n, const char* unit, int64_t unit_len,
                     std::string& out, int64_t* stats) {
    auto t0 = std::chrono::steady_clock::now();
    Graph g;
    g.k = k;
    for (int64_t i = 0; i < n; ++i) {          // :25-36 (in the caller's order: it fixes the node order)
        const std::string km(kmers + i * k, (size_t)k);
        g.add_edge(km.substr(0, (size_t)k - 1), km.substr(1), 0, true, km, counts[i]);
    }
    stats[0] = g.n_nodes; stats[1] = g.n_edges;
    g.collapse();
    stats[2] = g.n_nodes; stats[3] = g.n_edges;
    g.remove_tips();
    g.collapse();
    stats[4] = g.n_nodes; stats[5] = g.n_edges;
    g.purify(&stats[6]);
    stats[7] = g.n_nodes; stats[8] = g.n_edges;
    std::vector<int> le = g.live_edges();
    if (le.empty()) throw UsError{-64, "get_polished_unit: the purified graph has no edge (the reference fails on edges[0])"};
    int e0 = le[0];
    for (int e : le)
        if (g.tuple_less(e, e0)) e0 = e;
    const std::string& kmer = g.edges[(size_t)e0].kmer;
    const std::string cyc = kmer.substr(0, kmer.size() - (size_t)(k - 1));
    auto t1 = std::chrono::steady_clock::now();
    const std::string doubled = cyc + cyc, q(unit, (size_t)unit_len);
    int dist = 0, start = 0, end = 0;
    hw_first_location(q, doubled, &dist, &start, &end);
    out = doubled.substr((size_t)start, cyc.size());   // Python slicing: clipped at the end of the doubled unit
    auto t2 = std::chrono::steady_clock::now();
    stats[9] = (int64_t)cyc.size();
    stats[10] = dist;
    stats[11] = start;
    stats[12] = std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
    stats[13] = std::chrono::duration_cast<std::chrono::microseconds>(t2 - t1).count();
    return 0;
}

static void put_err(char* err, int errlen, const std::string& msg) {
    if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", msg.c_str());
}

}  // namespace

extern "C" int cfh_unit_star(int32_t k, const char* kmers, const int64_t* counts, int64_t n, const char* unit, int64_t unit_len,
                             char* out, int64_t cap, int64_t* out_len, int64_t* stats, char* err, int errlen) {
    int64_t st[CFH_UNIT_STAR_NSTATS] = {0};
    try {
        if (k < 2 || n < 0 || unit_len < 1 || (n > 0 && (!kmers || !counts)) || !unit || !out_len) {
            put_err(err, errlen, "cfh_unit_star: bad arguments (k >= 2, a non-empty unit)");
            return -22;
        }
        std::string res;
        unit_star(k, kmers, counts, n, unit, unit_len, res, st);
        if (stats) std::memcpy(stats, st, sizeof st);
        *out_len = (int64_t)res.size();
        if ((int64_t)res.size() > cap || (!out && cap > 0)) {
            put_err(err, errlen, "cfh_unit_star: output buffer too small");
            return -34;
        }
        if (!res.empty()) std::memcpy(out, res.data(), res.size());
        return 0;
    } catch (const UsError& e) {
        if (stats) std::memcpy(stats, st, sizeof st);
        put_err(err, errlen, e.msg);
        return e.code;
    } catch (const std::bad_alloc&) {
        put_err(err, errlen, "cfh_unit_star: out of memory");
        return -12;
    } catch (...) {
        put_err(err, errlen, "cfh_unit_star: internal error");
        return -5;
    }
}

extern "C" int cfh_hw_locate(const char* query, int64_t qlen, const char* target, int64_t tlen, int32_t out[3]) {
    try {
        if (!query || !target || !out || qlen < 1 || tlen < 1 || qlen > INT32_MAX || tlen > INT32_MAX) return -22;
        hw_first_location(std::string(query, (size_t)qlen), std::string(target, (size_t)tlen), &out[0], &out[1], &out[2]);
        return 0;
    } catch (const std::bad_alloc&) {
        return -12;
    } catch (...) {
        return -5;
    }
}
