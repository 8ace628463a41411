"""The de Bruijn graph on monostrings, the reads mapped to it, scaffolds and pseudounits: the drop-in for the reference's
``scripts/debruijn_graph.py`` as far as ``centroFlyeMono.py`` runs it, ``polish`` included (at the end of the file).  The hits of the reads on
the edges come from the device too (``Engine.monomap``, cf_monomap.hip); scaffolding and what follows it work on edge paths of a few
dozen elements and are host Python.

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

    def index_edges(self, min_k=2):
        """{k: {k-mer: (edge index, letter)}} for k = min_k .. self.k over the edges in ``edges()`` order, only the k-mers that occur
        exactly once; memoised in ``self.db_index``.  Host Python, for the API: ``map_reads`` does not use it."""
        if not hasattr(self, 'db_index'):
            seqs = [self.graph.data(*e)['edge_kmer'] for e in self.graph.edges()]
            self.db_index = {}
            for k in range(min_k, self.k + 1):
                places = {}
                for e_ind, seq in enumerate(seqs):
                    for j in range(len(seq) - k + 1):
                        places.setdefault(seq[j:j + k], []).append((e_ind, j))
                self.db_index[k] = {kmer: at[0] for kmer, at in places.items() if len(at) == 1}
        return self.db_index

    def map_reads(self, monoreads, gap_symb='?', verbose=True, engine=None):
        """{read id: (((edge index, letter), first read position), ((edge index, letter), last read position), valid path, [edges])} or
        None for a read without a hit: the hits of every read on the edge k-mers that occur exactly once, in one device call
        (``Engine.monomap``, cf_monomap.hip; the rule: include/cfhip.h).  Edges are numbered in ``edges()`` order.  ``self.db_index`` is
        neither built nor read."""
        from . import session
        engine = engine or session.engine()
        g = self.graph
        db_edges = g.edges()
        strings = _as_strings(monoreads)
        info, (ptr, path) = engine.monomap([g.data(*e)['edge_kmer'].encode('latin-1') for e in db_edges], [(u, v) for u, v, _ in db_edges],
                                           [s.encode('latin-1') for s in strings.values()], self.k, gap_symb.encode('latin-1'))
        ptr, path = ptr.tolist(), path.tolist()
        mapping = {}
        for x, (r_id, row) in enumerate(zip(strings, info.tolist())):
            if verbose:
                print(x + 1, len(strings))
            n_hits, e0, j0, i0, e1, j1, i1, valid, _ = row
            if n_hits == 0:
                mapping[r_id] = None
            else:
                mapping[r_id] = (((e0, j0), i0), ((e1, j1), i1), bool(valid), [db_edges[e] for e in path[ptr[x]:ptr[x + 1]]])
        return mapping


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


# ---------------------------------------------------------------- scaffolds and pseudounits (host Python: edge paths of a few dozen elements)
class OrderedDiGraph(OrderedMultiDiGraph):
    """The simple digraph of the scaffolding step: one edge per (u, v).  Its results depend on iteration orders of the graph library
    the reference uses, which are kept here: components by their first node in node order, each found breadth first over successors,
    then predecessors; the nodes of a component smaller than half the graph in the order of a set of them (built as that library
    builds it: from the search order, then once more from that set), else in node order; successors and predecessors in insertion
    order.  The nodes are tuples of ints, so the set's order is the same in every run."""

    def add_edge(self, u, v, **data):
        return OrderedMultiDiGraph.add_edge(self, u, v, key=0, **data)

    def components(self):
        seen, out = set(), []
        for n in self.succ:
            if n in seen:
                continue
            found, order, level = {n}, [n], [n]
            while level:
                nxt = []
                for x in level:
                    for y in list(self.succ[x]) + list(self.pred[x]):      # (no node is in both lists twice: found is checked)
                        if y not in found:
                            found.add(y)
                            nxt.append(y)
                            order.append(y)
                level = nxt
            comp = set(order)
            seen.update(comp)
            out.append(comp)
        return out

    def component_nodes(self, comp):
        shown = set(n for n in comp if n in self.succ)
        if 2 * len(shown) < len(self.succ):
            return [n for n in shown if n in self.succ]
        return [n for n in self.succ if n in shown]

    def topological_order(self, comp):
        """the component's nodes generation by generation, or None when it holds a cycle"""
        nodes = self.component_nodes(comp)
        waiting = {n: len(self.pred[n]) for n in nodes if self.pred[n]}
        level = [n for n in nodes if not self.pred[n]]
        order = []
        while level:
            nxt = []
            for n in level:
                order.append(n)
                for child in self.succ[n]:
                    waiting[child] -= 1
                    if waiting[child] == 0:
                        nxt.append(child)
                        del waiting[child]
            level = nxt
        return None if waiting else order

    def longest_path(self, order):
        """the longest path of a component given in topological order: per node the first best predecessor in predecessor order, the
        end the first farthest node in that order"""
        if not order:
            return []
        dist = {}
        for n in order:
            best = (0, n)
            froms = [(dist[p][0] + 1, p) for p in self.pred[n]]
            if froms:
                best = max(froms, key=lambda x: x[0])
            dist[n] = best
        at = max(dist, key=lambda n: dist[n][0])
        path, before = [], None
        while before != at:
            path.append(at)
            before, at = at, dist[at][1]
        return path[::-1]


def scaffolding(db, mappings, min_connections=2, additional_edges=list()):
    """(scaffold strings, scaffolds as edge lists): long (blue) edges that reads with a valid path connect at least min_connections
    times, chained along the longest path of every acyclic component of the connection graph, each link filled with its best
    supported path, and extended left and right by the longest read path.  No scaffold_graph.dot is written."""
    long_edges = list(db.get_long_edges())
    anchors = set(long_edges + list(additional_edges))
    valid_paths = [m[3] for m in mappings.values() if m is not None and m[2]]

    connections = {}
    for path in valid_paths:
        shared = set(path) & anchors
        if len(shared) > 1:
            at = sorted(path.index(e) for e in shared)
            for i, j in zip(at, at[1:]):
                support = connections.setdefault((path[i], path[j]), {})
                link = tuple(path[i:j + 1])
                support[link] = support.get(link, 0) + 1

    graph = OrderedDiGraph()
    for e in long_edges:
        graph.add_node(e)
    for (e1, e2), support in connections.items():
        if sum(support.values()) >= min_connections:
            graph.add_edge(e1, e2)

    edge_scaffolds = []
    for comp in graph.components():
        order = graph.topological_order(comp)
        if order is None:
            continue
        chain = graph.longest_path(order)
        scaffold = [chain[0]]
        for e1, e2 in zip(chain, chain[1:]):
            support = connections[(e1, e2)]
            scaffold += max(support, key=support.get)[1:]
        left, right = [], []
        for path in valid_paths:
            if chain[0] in path:
                ext = path[:path.index(chain[0])]
                if len(ext) > len(left):
                    left = ext
            if chain[-1] in path:
                ext = path[path.index(chain[-1]) + 1:]
                if len(ext) > len(right):
                    right = ext
        edge_scaffolds.append(list(left) + scaffold + list(right))
    return [db.get_path(s) for s in edge_scaffolds], edge_scaffolds


def read2scaffolds(db, scaffold_paths, mappings, monoreads):
    """{read id: (scaffold, first coordinate, last coordinate)} of the reads whose valid path fits exactly one place of one scaffold"""
    coords = [db.get_edgepath2coords(p) for p in scaffold_paths]
    places = {}
    for r_id, mapping in mappings.items():
        if mapping is None or not mapping[2]:
            continue
        ((_, j_st), _), ((_, j_en), _), _, read_path = mapping
        n = len(read_path)
        for s, scaffold in enumerate(scaffold_paths):
            for i in range(len(scaffold) - n + 1):
                if scaffold[i:i + n] == read_path:
                    places.setdefault(r_id, []).append((s, coords[s][i, j_st], coords[s][i + n - 1, j_en + db.k - 1]))
    return {r_id: at[0] for r_id, at in places.items() if len(at) == 1}


def cover_scaffolds_w_reads(r2s, mappings, scaffold_seqs, monoreads, k):
    """per scaffold and letter {read id: (monomer, st, en)}: the reads laid on their scaffold letter by letter through ``mono2nucl`` —
    as ``split_monostring`` leaves it, so a cut read covers what its truncated map still holds.  A read whose span on
    the scaffold and in itself differ is skipped."""
    coverage = [[{} for _ in seq] for seq in scaffold_seqs]
    for r_id, (s, s_st, s_en) in r2s.items():
        (_, r_st), (_, r_en), valid, _ = mappings[r_id]
        if not valid or s_en - s_st != r_en - r_st + k - 1:
            continue
        m2n = monoreads[r_id].mono2nucl
        for i in range(s_en - s_st + 1):
            if r_st + i in m2n:
                coverage[s][s_st + i][r_id] = m2n[r_st + i]
    return coverage


def partition_pseudounits(monostring):
    """[(st, en)]: the string cut greedily into stretches that hold no monomer twice"""
    units, st = [], 0
    while st < len(monostring):
        seen, en = set(), st
        while en < len(monostring) and monostring[en] not in seen:
            seen.add(monostring[en])
            en += 1
        units.append((st, en - 1))
        st = en
    return units


def extract_read_pseudounits(scaf_read_coverage, scaffold_seqs, monostrings, min_coverage=0):
    """(pseudounits per scaffold, per scaffold and kept pseudounit {read id: (st, en, strand)}): the reads that cover both ends of a
    pseudounit, with the nucleotide span between their two monomers"""
    pseudounits, read_pseudounits = [], []
    for seq, cov in zip(scaffold_seqs, scaf_read_coverage):
        units = partition_pseudounits(seq)
        pseudounits.append(units)
        per_unit = []
        for u_st, u_en in units:
            first, last = cov[u_st], cov[u_en]
            r_ids = set(first) & set(last)
            if len(r_ids) < min_coverage:
                continue
            spans = {}
            for r_id in r_ids:
                ends = first[r_id][1:] + last[r_id][1:]
                spans[r_id] = (min(ends), max(ends), monostrings[r_id].strand)
            per_unit.append(spans)
        read_pseudounits.append(per_unit)
    return pseudounits, read_pseudounits


# ---------------------------------------------------------------- polishing
class PolishError(RuntimeError):
    """polish refuses: nothing it wrote is left behind"""


_RC = str.maketrans('ATGCatgc-', 'TACGtacg-')


def RC(s):
    """the reference's reverse complement: ATGCatgc- swapped, every other byte as it is"""
    return s.translate(_RC)[::-1]


def _read_id(key):
    """the read a monostring key belongs to: a cut read is keyed (id, part)"""
    return key[0] if isinstance(key, tuple) else key


def _first_record(fn):
    """the sequence of the first FASTA record, its lines joined"""
    with open(fn) as f:
        blocks = f.read().split('>')[1:]
    if not blocks:
        raise PolishError(f'{fn} holds no record')
    return ''.join(blocks[0].split('\n')[1:]).replace('\r', '')


class _Tree:
    """the directories and files of one polish call: every file through .tmp and a rename, all of it gone again after rollback()"""

    def __init__(self):
        self.dirs, self.files = [], []

    def makedirs(self, path):
        missing = []
        while path and not os.path.isdir(path):
            missing.append(path)
            path = os.path.dirname(path)
        for d in reversed(missing):
            os.mkdir(d)
            self.dirs.append(d)

    def write(self, path, text):
        self.files.append(path)
        with open(path + '.tmp', 'w') as f:
            f.write(text)
        os.replace(path + '.tmp', path)

    def rollback(self):
        import shutil
        for fn in self.files:
            for p in (fn, fn + '.tmp'):
                if os.path.exists(p):
                    os.remove(p)
        for d in reversed(self.dirs):
            shutil.rmtree(d, ignore_errors=True)


def _fasta(records):
    return ''.join(f'>{name}\n{seq}\n' for name, seq in records.items())


def _monomer_template(scaffold, st, en, monomers, where):
    """the letters st .. en of the scaffold as nucleotides: the k-th monomer of the file is the k-th upper-case letter (SD_Report's
    monomer_names_map), a lower-case letter its reverse complement"""
    from string import ascii_lowercase, ascii_uppercase
    names = [name for name in monomers if not name.endswith("'")]
    upper = {c: monomers[name] for name, c in zip(names, ascii_uppercase)}
    lower = {c: RC(monomers[name]) for name, c in zip(names, ascii_lowercase)}
    out = []
    for c in scaffold[st:en + 1]:
        if c not in upper and c not in lower:
            raise PolishError(f'{where} has the letter {c!r}, which is no monomer')
        out.append(upper[c] if c in upper else lower[c])
    return ''.join(out)


def polish(scaffolds, pseudounits, read_pseudounits, reads, monomers, outdir, n_iter, n_threads, flye_bin='flye', *,
           polisher='flye', permille=300, uncovered='refuse', engine=None):
    """Every pseudounit polished with the stretches of the reads that cover it, and the polished pseudounits of a scaffold joined
    (the reference's ``polish``).  The export is the reference's, byte for byte: OUTDIR/scaffold_i/pseudounit_j/reads.fasta holds
    reads[read id][st:en + 1] of every covering read under the id s_{i}_t_{j}_{read id}_{st}_{en + 1}, reverse-complemented on strand
    '-', in the dict's order (a repeated id overwrites); template.fasta the first id in sorted order whose length is
    statistics.median_high of the lengths.  The read id of a key is key[0] for an (id, part) key and the key itself for a plain
    string (the reference takes r_id[0] either way: the first character of a plain id).

    polisher='flye' runs the reference's command per pseudounit (`flye_bin --nano-raw reads.fasta --polish-target template.fasta -i
    n_iter -t n_threads -o dir`, printed as the reference prints it) and reads polished_{n_iter}.fasta; a missing binary raises
    before anything is written, a missing polished file raises (the reference's fallback names an undefined variable).
    polisher='consensus' runs the built-in polisher once over all pseudounits of all scaffolds (``Engine.consensus_run``, n_iter
    passes, letters a .. z upper-cased for the run only), writes pseudounit_j/polished_k.fasta (>consensus_s_{i}_t_{j}_iter_{k}) for
    k = 1 .. n_iter, and files of this project: OUTDIR/consensus_report.tsv, OUTDIR/read_votes.tsv and
    scaffold_i/scaffold_i.support.tsv (formats: INTEGRATION.md).  Both write scaffold_i/scaffold_i.fasta (>scaffold_{i}_niter_{n_iter}).

    A pseudounit no read covers: uncovered='refuse' raises and names it (the reference dies in median_high([])); 'monomers' takes
    the concatenation of its letters' monomers as its sequence, unpolished.  Wherever the function raises — an uncovered
    pseudounit, a read id that `reads` lacks, a string beyond the consensus polisher's limit, a polisher that fails — nothing it
    wrote is left."""
    import shutil
    import statistics
    import subprocess
    if polisher not in ('flye', 'consensus'):
        raise ValueError("polisher is 'flye' or 'consensus'")
    if uncovered not in ('refuse', 'monomers'):
        raise ValueError("uncovered is 'refuse' or 'monomers'")
    if int(n_iter) < 1:
        raise PolishError('n_iter must be at least 1')
    if int(permille) < 0:
        raise PolishError('permille must not be negative')
    if polisher == 'flye' and shutil.which(str(flye_bin)) is None:
        raise PolishError(f"the Flye binary '{flye_bin}' was not found (flye_bin; or polisher='consensus', which needs none)")

    # the export, in memory: (i, j, {segment id: segment}, template id, template, covered)
    units = []
    for i, (scaffold, scaf_pseudounits) in enumerate(zip(scaffolds, pseudounits)):
        for j, (s_st, s_en) in enumerate(scaf_pseudounits):
            covering = read_pseudounits[i][j] if j < len(read_pseudounits[i]) else {}
            segments = {}
            for key, (r_st, r_en, strand) in covering.items():
                r_id = _read_id(key)
                if r_id not in reads:
                    raise PolishError(f'pseudounit {j} of scaffold {i}: the read {r_id!r} is not among the reads')
                segment = reads[r_id][r_st:r_en + 1]
                segments[f's_{i}_t_{j}_{r_id}_{r_st}_{r_en + 1}'] = RC(segment) if strand == '-' else segment
            if not segments:
                if uncovered == 'refuse':
                    raise PolishError(f"pseudounit {j} of scaffold {i} (letters {s_st} .. {s_en}) is covered by no read (uncovered='monomers' fills it from the monomers)")
                units.append((i, j, segments, f's_{i}_t_{j}_monomers', _monomer_template(scaffold, s_st, s_en, monomers, f'pseudounit {j} of scaffold {i}'), False))
                continue
            med_len = statistics.median_high([len(s) for s in segments.values()])
            template_id = next(s_id for s_id in sorted(segments) if len(segments[s_id]) == med_len)
            units.append((i, j, segments, template_id, segments[template_id], True))

    e = None
    if polisher == 'consensus':
        if engine is None:
            from . import session
            engine = session.engine()
        e = engine
        max_len = e.consensus_info()['max_len']
        for i, j, segments, _, template, _ in units:
            longest = max([len(template)] + [len(s) for s in segments.values()])
            if longest > max_len:
                raise PolishError(f"pseudounit {j} of scaffold {i} has a sequence of {longest} bases, more than the {max_len} polisher='consensus' takes")

    tree = _Tree()
    try:
        tree.makedirs(outdir)
        dirs = {}
        n_scaffolds = min(len(scaffolds), len(pseudounits))
        for i in range(n_scaffolds):
            tree.makedirs(os.path.join(outdir, f'scaffold_{i}'))
        polished = {}      # (i, j) -> the polished sequence
        for i, j, segments, template_id, template, covered in units:
            d = dirs[i, j] = os.path.join(outdir, f'scaffold_{i}', f'pseudounit_{j}')
            tree.makedirs(d)
            tree.write(os.path.join(d, 'reads.fasta'), _fasta(segments))
            tree.write(os.path.join(d, 'template.fasta'), _fasta({template_id: template}))
            if polisher == 'flye':
                if not covered:
                    polished[i, j] = template
                    continue
                cmd = [str(x) for x in (flye_bin, '--nano-raw', os.path.join(d, 'reads.fasta'), '--polish-target', os.path.join(d, 'template.fasta'),
                                        '-i', n_iter, '-t', n_threads, '-o', d)]
                print(' '.join(cmd))
                subprocess.check_call(cmd)
                fn = os.path.join(d, f'polished_{n_iter}.fasta')
                if not os.path.isfile(fn):
                    raise PolishError(f'pseudounit {j} of scaffold {i}: Flye left no {fn}')
                polished[i, j] = _first_record(fn)
        if polisher == 'consensus':
            _polish_consensus(tree, e, units, dirs, outdir, int(n_iter), int(permille), polished)
        for i in range(n_scaffolds):
            seq = ''.join(polished[i, j] for j in range(len(pseudounits[i])))
            tree.write(os.path.join(outdir, f'scaffold_{i}', f'scaffold_{i}.fasta'), _fasta({f'scaffold_{i}_niter_{n_iter}': seq}))
    except BaseException:
        tree.rollback()
        raise


def _polish_consensus(tree, e, units, dirs, outdir, n_iter, permille, polished):
    """one consensus_run over every pseudounit; polished_k.fasta, consensus_report.tsv, read_votes.tsv, scaffold_i.support.tsv"""
    up = lambda s: s.encode('latin-1').upper()      # noqa: E731  (bytes.upper touches a .. z only)
    templates = [up(t) for _, _, _, _, t, _ in units]
    flat = [up(s) for _, _, segments, _, _, _ in units for s in segments.values()]
    seg_ids = [s_id for _, _, segments, _, _, _ in units for s_id in segments]
    t_off = np.zeros(len(units) + 1, np.int64)
    np.cumsum([len(t) for t in templates], out=t_off[1:])
    pos_ptr = np.zeros(len(units) + 1, np.int64)
    np.cumsum([len(u[2]) for u in units], out=pos_ptr[1:])
    r_off = np.zeros(len(flat) + 1, np.int64)
    np.cumsum([len(r) for r in flat], out=r_off[1:])
    res = e.consensus_run(b''.join(templates), t_off, b''.join(flat), r_off, pos_ptr, n_iter, permille, support=True)
    per_read = [e.consensus_reads(k) for k in range(1, n_iter + 1)]
    agree = e.consensus_support(n_iter)
    report = ['scaffold\tunit\treads\ttemplate\ttemplate_length' + ''.join(f'\tlength_{k}\tvoting_{k}\texcluded_{k}' for k in range(1, n_iter + 1)) + '\tuncovered\n']
    votes, support = [], {}
    for x, (i, j, segments, template_id, template, covered) in enumerate(units):
        row = f'{i}\t{j}\t{len(segments)}\t{template_id}\t{len(template)}'
        for k, (b, off, n_voting, n_excluded) in enumerate(res, 1):
            text = b[off[x]:off[x + 1]].tobytes().decode('latin-1')
            tree.write(os.path.join(dirs[i, j], f'polished_{k}.fasta'), f'>consensus_s_{i}_t_{j}_iter_{k}\n{text}\n')
            row += f'\t{len(text)}\t{int(n_voting[x])}\t{int(n_excluded[x])}'
        polished[i, j] = text
        report.append(row + f'\t{int(not covered)}\n')
        for q in range(int(pos_ptr[x]), int(pos_ptr[x + 1])):
            votes.append(f'{i}\t{j}\t{seg_ids[q]}' + ''.join(f'\t{int(dist[q])}\t{int(voted[q])}' for dist, voted in per_read) + '\n')
        off, n_voting = res[-1][1], res[-1][2]
        lines = support.setdefault(i, [])
        for a in agree[off[x]:off[x + 1]].tolist():
            lines.append(f'{len(lines)}\t{j}\t{a}\t{int(n_voting[x])}\n')
    tree.write(os.path.join(outdir, 'consensus_report.tsv'), ''.join(report))
    tree.write(os.path.join(outdir, 'read_votes.tsv'), ''.join(votes))
    for i, lines in support.items():
        tree.write(os.path.join(outdir, f'scaffold_{i}', f'scaffold_{i}.support.tsv'), ''.join(lines))
