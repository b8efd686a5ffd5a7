"""TEST INFRASTRUCTURE ONLY -- stream capture through the HIP runtime itself
(ctypes), for tests/test_gpu_graph_capture.py: a stream of its own, capture
in hipStreamCaptureModeGlobal (the mode torch.cuda.graph and most callers
use), the captured graph's node types and edges, and replays.

torch.cuda.graph hides the graph; here it is looked at: a library call that
promises "no allocation, one linear launch sequence" must leave a chain of
kernel, memcpy and memset nodes and nothing else.
"""
import ctypes

import pytest

# hip_runtime_api.h: hipGraphNodeType, hipStreamCaptureMode, stream flags
KERNEL, MEMCPY, MEMSET = 0, 1, 2
MEM_ALLOC, MEM_FREE = 10, 11
CAPTURE_MODE_GLOBAL = 0
STREAM_NON_BLOCKING = 1
TYPE_NAMES = {0: "kernel", 1: "memcpy", 2: "memset", 3: "host", 4: "graph", 5: "empty", 6: "wait-event",
              7: "event-record", 10: "mem-alloc", 11: "mem-free"}


def _bind():
    import torch  # noqa: F401  (torch's HIP runtime is the one the library binds)
    h = ctypes.CDLL("libamdhip64.so.7")
    vp, sz, pvp = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)
    psz = ctypes.POINTER(sz)
    for name, args in (
            ("hipStreamCreateWithFlags", [pvp, ctypes.c_uint]),
            ("hipStreamDestroy", [vp]),
            ("hipStreamBeginCapture", [vp, ctypes.c_int]),
            ("hipStreamEndCapture", [vp, pvp]),
            ("hipGraphGetNodes", [vp, pvp, psz]),
            ("hipGraphNodeGetType", [vp, ctypes.POINTER(ctypes.c_int)]),
            ("hipGraphGetEdges", [vp, pvp, pvp, psz]),
            ("hipGraphInstantiate", [pvp, vp, pvp, ctypes.c_char_p, sz]),
            ("hipGraphLaunch", [vp, vp]),
            ("hipGraphExecDestroy", [vp]),
            ("hipGraphDestroy", [vp]),
            ("hipStreamSynchronize", [vp])):
        f = getattr(h, name)
        f.argtypes = args
        f.restype = ctypes.c_int
    return h


class Captured:
    """One captured graph: `types` (a node type per node), `edges` ((from, to)
    as node numbers), and its executable form once instantiate() has run."""

    def __init__(self, hip, stream, graph, types, edges):
        self.hip, self.stream, self.graph = hip, stream, graph
        self.types, self.edges = types, edges
        self.exe = None

    @property
    def nodes(self):
        return len(self.types)

    def names(self):
        return [TYPE_NAMES.get(t, str(t)) for t in self.types]

    def is_linear_chain(self):
        """edges == nodes - 1 and no node with two predecessors or two
        successors: with no cycles in a graph, one chain."""
        n = self.nodes
        ins, outs = [0] * n, [0] * n
        for a, b in self.edges:
            outs[a] += 1
            ins[b] += 1
        return n > 0 and len(self.edges) == n - 1 and max(ins) <= 1 and max(outs) <= 1

    def instantiate(self):
        exe = ctypes.c_void_p()
        rc = self.hip.hipGraphInstantiate(ctypes.byref(exe), self.graph, None, None, 0)
        assert rc == 0 and exe.value, "hipGraphInstantiate: %d" % rc
        self.exe = exe
        return self

    def launch(self):
        assert self.exe is not None, "a graph is launched only after a capture that succeeded"
        rc = self.hip.hipGraphLaunch(self.exe, self.stream)
        assert rc == 0, "hipGraphLaunch: %d" % rc

    def destroy(self):
        if self.exe is not None:
            self.hip.hipGraphExecDestroy(self.exe)
            self.exe = None
        if self.graph is not None:
            self.hip.hipGraphDestroy(self.graph)
            self.graph = None


class GraphStream:
    """A non-blocking stream of its own with capture(), as the raw handle
    (`handle`, for the C-ABI) and as a torch stream (`torch_stream`, for
    stream-ordered copies and fills between replays)."""

    def __init__(self):
        import torch
        self.hip = _bind()
        s = ctypes.c_void_p()
        rc = self.hip.hipStreamCreateWithFlags(ctypes.byref(s), STREAM_NON_BLOCKING)
        assert rc == 0 and s.value, "hipStreamCreateWithFlags: %d" % rc
        self.handle = s
        self.torch_stream = torch.cuda.ExternalStream(s.value)

    def synchronize(self):
        rc = self.hip.hipStreamSynchronize(self.handle)
        assert rc == 0, "hipStreamSynchronize: %d" % rc

    def close(self):
        if self.handle is not None:
            self.hip.hipStreamSynchronize(self.handle)
            self.hip.hipStreamDestroy(self.handle)
            self.handle = None

    def capture(self, fn, want=0):
        """Captures what fn() enqueues on the stream (Global mode).  fn returns
        the library's return code, which must be `want`.  Whatever fails, the
        capture is ended and what exists of the graph destroyed before the
        test fails with the code: a graph whose capture failed is never
        launched."""
        hip = self.hip
        rc = hip.hipStreamBeginCapture(self.handle, CAPTURE_MODE_GLOBAL)
        if rc != 0:
            pytest.fail("hipStreamBeginCapture: %d" % rc)
        graph = ctypes.c_void_p()
        got, err = None, None
        try:
            got = fn()
        except BaseException as e:  # noqa: B036  (the capture must end whatever happened)
            err = e
        end = hip.hipStreamEndCapture(self.handle, ctypes.byref(graph))
        if err is not None or got != want or end != 0 or not graph.value:
            if graph.value:
                hip.hipGraphDestroy(graph)
            if err is not None:
                raise err
            pytest.fail("capture failed: the call returned %r (want %r), hipStreamEndCapture %d" % (got, want, end))
        cap = None
        try:
            cap = self._inspect(graph)
        finally:
            if cap is None:
                hip.hipGraphDestroy(graph)
        return cap

    def _inspect(self, graph):
        hip = self.hip
        n = ctypes.c_size_t(0)
        rc = hip.hipGraphGetNodes(graph, None, ctypes.byref(n))
        assert rc == 0, "hipGraphGetNodes: %d" % rc
        nodes = (ctypes.c_void_p * max(n.value, 1))()
        if n.value:
            rc = hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n))
            assert rc == 0, "hipGraphGetNodes: %d" % rc
        number = {nodes[i]: i for i in range(n.value)}
        types = []
        for i in range(n.value):
            t = ctypes.c_int(-1)
            rc = hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t))
            assert rc == 0, "hipGraphNodeGetType: %d" % rc
            types.append(t.value)
        ne = ctypes.c_size_t(0)
        rc = hip.hipGraphGetEdges(graph, None, None, ctypes.byref(ne))
        assert rc == 0, "hipGraphGetEdges: %d" % rc
        frm = (ctypes.c_void_p * max(ne.value, 1))()
        to = (ctypes.c_void_p * max(ne.value, 1))()
        if ne.value:
            rc = hip.hipGraphGetEdges(graph, frm, to, ctypes.byref(ne))
            assert rc == 0, "hipGraphGetEdges: %d" % rc
        edges = [(number[frm[i]], number[to[i]]) for i in range(ne.value)]
        return Captured(hip, self.handle, graph, types, edges)
