"""Values handed from one autograd function to another beside the autograd edges: bounded tables keyed by a tensor's address.

An address names a tensor only while that tensor lives and is unchanged: the caching allocator gives a freed address to the
next tensor, and kernels write through raw pointers.  So an entry left under tensor t is returned for a lookup tensor x only if
  * the anchor is alive: a weak reference to t (an entry nobody claims pins no memory) or, with held=True, a detached alias
    of t (same storage and version counter: the address is not reused while the entry lives, t's autograd graph is not pinned);
  * x has t's shape and strides, and the version recorded at put() is the anchor's and x's now (no in-place write since);
  * same(t) at put() equals same(x) at get(), where the table has one (a mask's side of a graph capture; id for "this object").
An entry found invalid is deleted.  A kernel that writes through a raw pointer moves no version: its caller says drop().
At its bound a table first drops the entries that cannot become valid again (anchor dead, version moved), then the oldest -
except with evict_live=False, where a live entry is never evicted (it is still owed to somebody).
ops.py declares the tables (statistics, masks, sites, twins, gradients) and what empties each.  Host code only, no flags."""
import weakref


class Handover:
    def __init__(self, name, bound=None, held=False, same=None, evict_live=True):
        self.name, self.bound, self.held, self.same, self.evict_live = name, bound, held, same, evict_live
        self._d = {}        # address -> (anchor, version, same(t), value, keep), oldest first

    def _valid(self, e, x=None):        # the anchor lives at the recorded version - and x, where given, is that tensor as it was
        a = e[0] if self.held else e[0]()
        return a is not None and a._version == e[1] and (x is None or (
            x._version == e[1] and a.shape == x.shape and a.stride() == x.stride()
            and (self.same is None or self.same(x) == e[2])))

    def put(self, t, value, keep=False):
        """-> t.  keep: get() hands the value out every time (until drop / clear), else once"""
        d = self._d
        d.pop(t.data_ptr(), None)
        if self.bound is not None and len(d) >= self.bound:
            d = self._d = {k: e for k, e in d.items() if self._valid(e)}
            while self.evict_live and len(d) >= self.bound:
                del d[next(iter(d))]
        d[t.data_ptr()] = (t.detach() if self.held else weakref.ref(t), t._version, self.same and self.same(t), value, keep)
        return t

    def get(self, x, pop=True):
        """the value left under x, else None; pop=False leaves a valid entry in place"""
        e = self._d.get(x.data_ptr())
        if e is None:
            return None
        ok = self._valid(e, x)
        if not ok or (pop and not e[4]):
            del self._d[x.data_ptr()]
        return e[3] if ok else None

    def drop(self, t):
        self._d.pop(t.data_ptr(), None)

    def clear(self, kept=False):        # kept: the entries put with keep=True stay
        self._d = {k: e for k, e in self._d.items() if kept and e[4]}

    def __len__(self):
        return len(self._d)

    def __contains__(self, address):
        return address in self._d
