"""The hipGraph replay protocol of the predictors (infer.Predictor, ensemble.EnsemblePredictor): per key one warm-up call, one capturing
call, then replays out of a static input buffer; at most max_graphs keys are kept, least recently used first out.

    cache = ReplayCache("infer", max_graphs=4)
    out = cache(key, src, run)                   # run(src) on the warm-up call, afterwards the static output of the key's graph

The caller brings its weights up to date and holds torch.no_grad() around the call; run must launch the same kernels for the same key.
"""
import collections
import itertools

import torch

from . import ops

_serial = itertools.count()


class ReplayCache:
    def __init__(self, prefix, max_graphs=4):
        self.prefix = prefix
        self.max_graphs = max(1, int(max_graphs))
        self.num_captures = 0
        self.entries = collections.OrderedDict()     # key -> {"tag", "graph", "src", "out"}, least recently used first

    def __call__(self, key, src, run):
        ent = self.entries.get(key)
        if ent is None:
            while len(self.entries) >= self.max_graphs:
                self.drop(next(iter(self.entries)))
            tag = (self.prefix, next(_serial))       # never reused (id() of a dead owner would hand its stale tables to a new one)
            try:
                with ops.table_namespace(tag):       # warm-up: allocator, device tables, lazy kernel attributes, cast-weight caches
                    out = run(src)
            except BaseException:
                ops.drop_table_namespace(tag)
                raise
            self.entries[key] = {"tag": tag, "graph": None, "src": None, "out": None}    # only a key that warmed up is captured
            return out
        self.entries.move_to_end(key)
        if ent["graph"] is None or ent["src"].shape != src.shape or ent["src"].dtype != src.dtype:
            ent["graph"] = None
            ent["src"] = src.detach().clone(memory_format=torch.contiguous_format)
            g = torch.cuda.CUDAGraph(keep_graph=True)                  # the graph stays inspectable (raw_cuda_graph: kernel-node counts)
            with ops.table_namespace(ent["tag"]), torch.cuda.graph(g):
                ent["out"] = run(ent["src"])
            g.instantiate()
            ent["graph"] = g
            self.num_captures += 1
        else:
            ent["src"].copy_(src)
        ent["graph"].replay()
        return ent["out"]

    def drop(self, key):
        ent = self.entries.pop(key)
        ent["graph"] = None
        ops.drop_table_namespace(ent["tag"])

    def reset(self):
        for key in list(self.entries):
            self.drop(key)
