"""`CapturedStep` — one device step captured into a hipGraph, repaired and instantiated, with everything that goes with it.

On this ROCm a captured hipMemsetAsync takes effect on the first launch only, and ATen's split reductions (every nn.Linear's
bias gradient) zero their semaphores with one.  So a capture keeps its graph (`keep_graph=True`), has its memset nodes
rewritten into fill kernels (csrc/graph_fix.hip), refuses a graph with a pitched memset left in it, and is instantiated only
after that: one that misses any of these trains wrong from the second replay on."""
import torch

from asac_amd import native


class CapturedStep:
    __slots__ = ('graph', 'exec_handle', 'watched', 'memsets', 'payload', '_device')

    def __init__(self, graph, memsets, payload, device, exec_handle=None):
        self.graph, self._device = graph, device      # (an instantiated torch.cuda.CUDAGraph)
        self.exec_handle = exec_handle  # the raw hipGraphExec_t once the graph may be launched past torch (`replay`)
        self.watched = False            # the first replay went through torch and watched its generator
        self.memsets = memsets          # (replaced, kept) of the memset-node pass
        self.payload = payload          # what the owner keeps with the graph: `fn`'s return value until it stores its own

    @staticmethod
    def api_ok() -> bool:
        """`CUDAGraph(keep_graph=True)` / `raw_cuda_graph()` / `instantiate()`: the memset-node repair needs the graph before
        instantiation.  A torch build without them cannot replay a captured step correctly here."""
        import inspect
        try:
            return ('keep_graph' in inspect.signature(torch.cuda.CUDAGraph.__new__).parameters or
                    'keep_graph' in (torch.cuda.CUDAGraph.__new__.__doc__ or '') or
                    hasattr(torch.cuda.CUDAGraph, 'raw_cuda_graph')) and hasattr(torch.cuda.CUDAGraph, 'instantiate')
        except (TypeError, ValueError):
            return hasattr(torch.cuda.CUDAGraph, 'raw_cuda_graph') and hasattr(torch.cuda.CUDAGraph, 'instantiate')

    @classmethod
    def capture(cls, fn, device, take_exec: bool = False, logger=None) -> 'CapturedStep':
        """Capture `fn()` on a side stream -> an executable graph.  Raises where the capture, the repair or the instantiation
        does: what a failure means is the caller's business.  `take_exec`: take the raw handle at once — for a step already
        known to draw no torch random numbers (`replay`)."""
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        # thread_local: the RCCL watchdog thread may query events while this thread captures
        with torch.cuda.graph(graph, stream=side, capture_error_mode='thread_local'):
            payload = fn()
        replaced, kept = native.graph_replace_memset_nodes(int(graph.raw_cuda_graph()))
        if kept:
            # a pitched (2-D) memset has the same replay fault the pass exists to repair and is not rewritten: a step that
            # captured one must not be replayed (no kernel of the library or of ATen's step issues one today)
            raise RuntimeError(f'{kept} 2-D memset node(s) in the captured step: not replayable on this ROCm')
        graph.instantiate()
        torch.cuda.current_stream().wait_stream(side)
        if replaced and logger is not None:
            logger.info(f'captured graph: {replaced} memset node(s) replaced by fill kernels')
        return cls(graph, (replaced, kept), payload, device, int(graph.raw_cuda_graph_exec()) if take_exec else None)

    def replay(self, direct: bool = True, logger=None) -> None:
        """torch's `CUDAGraph.replay()` re-seeds its Philox generator before every launch (two fill kernels).  The first
        replay goes through torch and watches the generator offset: if the captured step consumed no torch random numbers
        (all draws come from `asac_noise_fill`), later steps launch the instantiated graph directly.  `direct=False`: never."""
        if self.exec_handle is not None:
            native.graph_launch(self.exec_handle)
            return
        if self.watched or not direct:
            self.graph.replay()
            return
        gen = torch.cuda.default_generators[self._device.index or 0]
        before = gen.get_offset()
        self.graph.replay()
        self.watched = True
        if gen.get_offset() == before and hasattr(self.graph, 'raw_cuda_graph_exec'):
            try:
                self.exec_handle = int(self.graph.raw_cuda_graph_exec())
                if logger is not None:
                    logger.info('captured step draws no torch random numbers: launching the graph directly')
            except Exception as e:   # older torch: keep torch's replay
                if logger is not None:
                    logger.warning(f'raw graph handle unavailable, using CUDAGraph.replay(): {e!r}')
