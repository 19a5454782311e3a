"""`model(images)` of a fixed input shape as one HIP-graph launch (`SSDModel.graphed`)."""
import torch

from ._conv_select import switch


class GraphedInference:
    """`model(images)` (forward + DecodeDetections) of a fixed input shape as a HIP graph.

    The graph reads the tensor handed to the constructor (`static_in`) and writes `static_out`: calling the object with another
    tensor copies it into `static_in` first (one device copy); the returned tensor is overwritten by the next call.  Capture happens
    after `warmup` eager steps on the capture stream, so the per-shape kernel autotune, the workspaces and the side stream of the
    predictor heads exist before anything is recorded (allocations, host -> device copies and timing syncs are illegal inside a
    capture).  Inference only (no_grad)."""

    def __init__(self, model, images, warmup=3, fn=None):
        if not images.is_cuda:
            raise ValueError("HIP graphs need a CUDA/HIP tensor")
        run = fn if fn is not None else model            # fn: another callable of the model on the same input (model.head_outputs)
        self.model = model
        self.static_in = images
        dev = images.device
        self.stream = torch.cuda.Stream(device=dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        had = model.__dict__.get("_head_overlap")
        model.__dict__["_head_overlap"] = switch("GRAPH_HEAD_OVERLAP")   # two streams inside the graph: explicit dependencies, no allocator subtleties
        try:
            with torch.cuda.stream(self.stream), torch.no_grad():
                for _ in range(max(1, warmup)):
                    run(self.static_in)
            torch.cuda.current_stream(dev).wait_stream(self.stream)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="relaxed"):
                self.static_out = run(self.static_in)
        finally:
            model.__dict__["_head_overlap"] = had
        # (see __call__: an OLDER graph of a model must not be replayed on a foreign stream once a newer one exists)
        self._epoch = model.__dict__.get("_graph_epoch", 0) + 1
        model.__dict__["_graph_epoch"] = self._epoch

        # What the recorded kernels read besides `static_in`: the parameters' own storage (in-place updates -- optimizer steps,
        # load_state_dict, load_keras_weights -- are seen by the next replay) and the PACKED head filters, separate tensors built from
        # the conf / loc weights, and the other tensors DERIVED from parameters (the fragment-packed conv7_1 ... conv9_2 filters of
        # SSD300's one-launch tail, the float32 copy of L2Normalization's gamma in a bf16 model): all of them are refreshed in place
        # when the parameter they come from changed (`_refresh_derived_weights`, keyed on `_derived_weights_key`).  A parameter
        # whose storage was REPLACED (`conv.weight = nn.Parameter(...)`, `param.data = t`) is something the graph cannot follow.
        self._param_ptrs = tuple(p.data_ptr() for p in model.parameters())
        self._derived_key = model._derived_weights_key()

    def __call__(self, images=None):
        if images is not None and images.data_ptr() != self.static_in.data_ptr():
            if tuple(images.shape) != tuple(self.static_in.shape) or images.dtype != self.static_in.dtype:
                raise ValueError("this graph was captured for images of shape %s / %s, got %s / %s" % (
                    tuple(self.static_in.shape), self.static_in.dtype, tuple(images.shape), images.dtype))
            self.static_in.copy_(images, non_blocking=True)
        if tuple(p.data_ptr() for p in self.model.parameters()) != self._param_ptrs:
            raise RuntimeError("a parameter's storage was replaced after the graph was captured: call model.graphed(...) again")
        key = self.model._derived_weights_key()
        if key != self._derived_key:
            self.model._refresh_derived_weights()
            self._derived_key = key
        cur = torch.cuda.current_stream(self.static_in.device)
        if self.model.__dict__.get("_graph_epoch", 0) != self._epoch and cur.cuda_stream != self.stream.cuda_stream:
            # Another graph of this model was captured after this one.  On ROCm 7.2 replaying the OLDER of two such graphs on a stream
            # other than its capture stream segfaults inside hipGraphLaunch (tools/debug_two_graphs.py: 2 graphs + foreign stream
            # crashes, 1 graph or the capture stream does not; profiles/r06zq_two_steps_in_flight_negative.txt) -- so it is replayed
            # on its capture stream, ordered behind and in front of the caller's stream.
            self.stream.wait_stream(cur)
            with torch.cuda.stream(self.stream):
                self.graph.replay()
            cur.wait_stream(self.stream)
            return self.static_out
        self.graph.replay()
        return self.static_out
