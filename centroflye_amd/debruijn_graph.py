"""The de Bruijn graph on monostrings up to its contigs: the drop-in for the part of the reference's ``scripts/debruijn_graph.py``
that ``centroFlyeMono.py`` runs up to ``iterative_graph`` (mapping, scaffolding, pseudounits and polishing are not here).

The k-mer counts — every gap-free window of k letters over all strings, counted exactly, in the order of first occurrence — come
from the device (``Engine.monokmers``, cf_monokmers.hip); the reference slices a k-letter string at every position in Python.  The
k-mer strings are cut from the first occurrences only.

The graph is a small ordered multigraph of our own (``OrderedMultiDiGraph``).  The reference's results depend on the iteration
orders of the graph library it uses, so the orders are those of insertion-ordered dicts: nodes in the order ``add_edge`` first saw
them (u before v), ``edges()`` by node, then successor, then key, ``in_edges`` from the predecessor map, ``reverse()`` adds all
nodes and then the edges in ``edges()`` order, and ``remove_node`` / later ``add_edge`` calls shift the orders as dict deletion and
insertion do.  Two oddities of the reference shape results and are kept: a lone cycle next to other nodes removes itself when the
paths are collapsed (its last node sees one edge in and one out, the merged edge is added to that node, and the node goes), and
the set of taken edges of the out-path walk is shared by all walks of one pass.

Differences, on purpose: ``get_contigs`` returns its contigs SORTED and its paths in the order they were first found (the reference
returns both in the order of a set of strings or tuples, which no run fixes); ``iterative_graph`` creates ``outdir`` but writes no
``.dot`` files."""
import os
from collections import Counter

import numpy as np


class OrderedMultiDiGraph:
    """Directed multigraph with the iteration orders described in the module docstring.  An edge is (u, v, key); its data is a dict."""

    def __init__(self):
        self.succ = {}      # u -> {v -> {key -> data}}
        self.pred = {}      # v -> {u -> {key -> data}} (the same data objects)

    def add_node(self, n):
        if n not in self.succ:
            self.succ[n] = {}
            self.pred[n] = {}

    def add_edge(self, u, v, key=None, **data):
        self.add_node(u)
        self.add_node(v)
        keys = self.succ[u].get(v)
        if keys is None:
            keys = {}
            self.succ[u][v] = keys
            self.pred[v][u] = keys
        if key is None:
            key = len(keys)
            while key in keys:
                key += 1
        keys[key] = data
        return key

    def remove_node(self, n):
        for v in list(self.succ[n]):
            del self.pred[v][n]
        for u in list(self.pred[n]):
            del self.succ[u][n]
        del self.succ[n]
        del self.pred[n]

    def nodes(self):
        return list(self.succ)

    def number_of_nodes(self):
        return len(self.succ)

    def edges(self):
        return [(u, v, key) for u, nbrs in self.succ.items() for v, keys in nbrs.items() for key in keys]

    def out_edges(self, n):
        return [(n, v, key) for v, keys in self.succ[n].items() for key in keys]

    def in_edges(self, n):
        return [(u, n, key) for u, keys in self.pred[n].items() for key in keys]

    def out_degree(self, n):
        return sum(len(keys) for keys in self.succ[n].values())

    def in_degree(self, n):
        return sum(len(keys) for keys in self.pred[n].values())

    def data(self, u, v, key):
        return self.succ[u][v][key]

    def reverse(self):
        rev = OrderedMultiDiGraph()
        for n in self.succ:
            rev.add_node(n)
        for u, v, key in self.edges():
            rev.add_edge(v, u, key=key, **self.succ[u][v][key])
        return rev

    def weak_components(self):
        """the node sets of the weakly connected components, by their first node in node order"""
        seen, out = set(), []
        for n in self.succ:
            if n in seen:
                continue
            comp, todo = {n}, [n]
            while todo:
                x = todo.pop()
                for y in list(self.succ[x]) + list(self.pred[x]):
                    if y not in comp:
                        comp.add(y)
                        todo.append(y)
            seen |= comp
            out.append(comp)
        return out


class DeBruijnGraph:
    def __init__(self, k, max_uniq_cov=60, min_uniq_len=1000):
        self.graph = OrderedMultiDiGraph()
        self.k = k
        self.node_mapping = {}
        self.rev_node_mapping = {}
        self.max_uniq_cov = max_uniq_cov
        self.min_uniq_len = min_uniq_len

    def _node(self, label):
        if label not in self.node_mapping:
            self.rev_node_mapping[len(self.node_mapping)] = label
            self.node_mapping[label] = len(self.node_mapping)
        return self.node_mapping[label]

    def add_kmer(self, kmer, coverage=1):
        u = self._node(kmer[:-1])
        v = self._node(kmer[1:])
        self.graph.add_edge(u, v, edge_kmer=kmer, length=1, coverages=[coverage], color='black')

    def add_kmers(self, kmers, coverage=None):
        for kmer in kmers:
            if coverage is None:
                self.add_kmer(kmer)
            else:
                self.add_kmer(kmer, coverage=coverage[kmer])

    def collapse_nonbranching_paths(self):
        g = self.graph
        for node in g.nodes():
            if g.number_of_nodes() > 1 and g.in_degree(node) == 1 and g.out_degree(node) == 1:
                (src, _, key_in), (_, dst, key_out) = g.in_edges(node)[0], g.out_edges(node)[0]
                into, out = g.data(src, node, key_in), g.data(node, dst, key_out)
                kmer = into['edge_kmer'] + out['edge_kmer'][self.k - 1:]
                coverages = sorted(into['coverages'] + out['coverages'])
                unique = len(coverages) + self.k - 1 >= self.min_uniq_len and np.median(coverages) <= self.max_uniq_cov
                g.add_edge(src, dst, edge_kmer=kmer, coverages=coverages, length=len(coverages), color='blue' if unique else 'black')
                g.remove_node(node)

    def get_edges(self):
        self.collapse_nonbranching_paths()
        g = self.graph
        datas = [g.data(*e) for e in g.edges()]
        return [d['edge_kmer'] for d in datas], [np.median(d['coverages']) for d in datas]

    def get_path(self, list_edges):
        path = self.graph.data(*list_edges[0])['edge_kmer']
        for edge in list_edges[1:]:
            seq = self.graph.data(*edge)['edge_kmer']
            assert path[-(self.k - 1):] == seq[:self.k - 1]
            path += seq[self.k - 1:]
        if list_edges[0][0] == list_edges[-1][1]:      # a cycle: its last k - 1 letters are its first
            path = path[:-(self.k - 1)]
        return path

    def get_edgepath2coords(self, list_edges):
        """{(edge number in the path, letter of the edge): coordinate in get_path's string, edge number: where its successor starts}"""
        coords = {}
        at = 0
        path = self.get_path(list_edges)
        for i, edge in enumerate(list_edges):
            seq = self.graph.data(*edge)['edge_kmer']
            for j, letter in enumerate(seq):
                assert path[at] == letter
                coords[(i, j)] = at
                at += 1
            at -= self.k - 1
            coords[i] = at
        return coords

    @staticmethod
    def _longest_valid_outpaths(graph):
        taken = set()      # shared by every walk of this pass, as in the reference

        def walk(edge):
            path = [edge]
            while graph.out_degree(edge[1]) == 1:
                nxt = graph.out_edges(edge[1])[0]
                if nxt in taken:
                    break
                taken.add(edge)
                path.append(nxt)
                edge = nxt
            return path

        outpaths = {}
        for edge in graph.edges():
            if edge not in outpaths:
                outpaths[edge] = walk(edge)
                for i, e in enumerate(outpaths[edge][1:]):
                    outpaths[e] = outpaths[edge][i + 1:]
        return outpaths

    def get_contigs(self):
        self.collapse_nonbranching_paths()
        outpaths = self._longest_valid_outpaths(self.graph)
        inpaths = {}
        for (v, u, key), path in self._longest_valid_outpaths(self.graph.reverse()).items():
            inpaths[(u, v, key)] = [(b, a, c) for a, b, c in reversed(path)]
        found = {}
        for edge, outpath in outpaths.items():
            path = inpaths[edge]
            seen = set(path)
            for e in outpath[1:]:
                if e in seen:
                    break
                path.append(e)
                seen.add(e)
            found[tuple(path)] = None
        found = list(found)

        def inside(short, long):
            return any(short == long[i:i + len(short)] for i in range(len(long) - len(short) + 1))

        paths = [p for p in found if not any(p != q and inside(p, q) for q in found)]
        contigs = sorted({self.get_path(p) for p in paths})
        return contigs, paths

    def get_long_edges(self):
        g = self.graph
        return {e: g.data(*e)['edge_kmer'] for e in g.edges() if g.data(*e)['color'] == 'blue'}


def _as_strings(strings):
    """{id: str} of a dict of strings or MonoStrings"""
    return {r_id: s if isinstance(s, str) else s.tostring() for r_id, s in strings.items()}


def _count(strings, k, min_mult, gap_symb, positions, engine=None):
    """Engine.monokmers over the dict's strings -> ({k-mer: count} in the order of first occurrence, {k-mer: [(id, i)]} or None)"""
    from . import session
    engine = engine or session.engine()
    strings = _as_strings(strings)
    ids = list(strings)
    encoded = [s.encode('latin-1') for s in strings.values()]
    res = engine.monokmers(encoded, k, min_mult, positions, gap_symb.encode('latin-1'))
    first = res[0] if positions else res
    counts = {}
    for s, i, count, _ in first.tolist():
        counts[strings[ids[s]][i:i + k]] = count
    if not positions:
        return counts, None
    _, ptr, occ = res
    pairs = list(zip((ids[s] for s in occ['s'].tolist()), occ['i'].tolist()))
    return counts, {kmer: pairs[ptr[j]:ptr[j + 1]] for j, kmer in enumerate(counts)}


def get_all_kmers(strings, k, gap_symb='?'):
    counts, where = _count(strings, k, 1, gap_symb, True)
    return Counter(counts), where


def get_frequent_kmers(strings, k, min_mult=5):
    return _count(strings, k, min_mult, '?', True)


def get_complex_nodes(graph):
    return [n for n in graph.nodes() if graph.in_degree(n) > 1 and graph.out_degree(n) > 1]


def get_paths_thru_complex_nodes(db, strings, min_mult=2):
    g, k = db.graph, db.k
    nodes = get_complex_nodes(g)
    if not nodes:
        return {}
    counts, _ = _count(strings, k + 1, min_mult, '?', False)      # one call; every (k + 1)-mer below min_mult is left out by it
    selected = {}
    for node in nodes:
        for into in g.in_edges(node):
            for out in g.out_edges(node):
                in_kmer, out_kmer = g.data(*into)['edge_kmer'][-k:], g.data(*out)['edge_kmer'][:k]
                assert in_kmer[1:] == out_kmer[:-1]
                kp1 = in_kmer + out_kmer[-1]
                if kp1 in counts:
                    selected[kp1] = counts[kp1]
    return selected


def iterative_graph(monostrings, min_k, max_k, outdir, min_mult=5, step=1, starting_graph=None, verbose=True):
    os.makedirs(outdir, exist_ok=True)
    dbs, all_contigs, all_frequent, all_positions = {}, {}, {}, {}
    strings = _as_strings(monostrings)
    input_strings = dict(strings)
    complex_kp1mers = {}

    def with_contigs(contigs, k):
        out = dict(strings)
        for i, contig in enumerate(contigs):
            for j in range(min_mult):
                out[f'contig_k{k}_i{i}_j{j}'] = contig
        return out

    if starting_graph is not None:
        input_strings = with_contigs(starting_graph.get_contigs()[0], min_k)
        complex_kp1mers = get_paths_thru_complex_nodes(starting_graph, strings)

    for k in range(min_k, max_k + 1, step):
        frequent, positions = get_frequent_kmers(input_strings, k=k, min_mult=min_mult)
        frequent.update(complex_kp1mers)
        if verbose:
            print(f'\nk={k}')
            print(f'#frequent kmers = {len(frequent)}')
        all_frequent[k], all_positions[k] = frequent, positions
        db = DeBruijnGraph(k=k)
        db.add_kmers(frequent, coverage=frequent)
        db.collapse_nonbranching_paths()
        if verbose:
            comps = db.graph.weak_components()
            if len(comps) > 1:
                print(f'#cc = {len(comps)}')
                for comp in comps:
                    print(len(comp))
        dbs[k] = db
        contigs, _ = db.get_contigs()
        all_contigs[k] = contigs
        input_strings = with_contigs(contigs, k)
        complex_kp1mers = get_paths_thru_complex_nodes(db, strings)
    return all_contigs, dbs, all_frequent, all_positions
