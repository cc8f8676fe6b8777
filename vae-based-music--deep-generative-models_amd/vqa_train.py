"""What the VQ-VAE and prior trainers share: the train step as a replayable hipGraph, the optimizer's half of a
checkpoint, and the context in which a model runs on the moving average of its weights. What differs between the models stays with them: their inputs and checks, and what surrounds a replay."""
from __future__ import annotations

import gc
from contextlib import contextmanager

import torch

import vqa_dp


class CapturedStep:
    """One train step built from a model's own bound methods: compute() (forward + backward into the bucket),
    exchange() (the data-parallel sum), update() (optimizer + trackers) and, if it trains from a device feed, the feed
    (next() launches the batch gather and advances the device step counter; `seed` is what that launch holds).
    warm_up(n), then capture(): `graphs` is then (g1, g2), g2 None in the one-graph form, and replay() runs the step."""

    def __init__(self, device, process_group, feed, compute, exchange, update):
        self.device, self.process_group, self.feed = device, process_group, feed
        self.feed_seed = feed.seed if feed is not None else None
        self.draw = feed.next if feed is not None else (lambda: None)
        self.compute, self.exchange, self.update = compute, exchange, update

    def warm_up(self, steps):
        """`steps` real eager steps on a side stream, joined back into the current stream, then a synchronise."""
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(steps):
                self.draw()
                self.compute()
                self.exchange()
                self.update()
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)

    def capture(self, exchange_captured=lambda: False):
        """ONE graph (draw, compute, [exchange], update) when the step has no exchange (no data parallelism) or
        exchange_captured(), read after compute has run inside the capture, says the exchange runs on the device;
        otherwise TWO graphs (draw + compute, update) around the eager exchange."""
        # A model and its CapturedStep refer to each other, so a dropped model (its hipGraphs, events and pool memory)
        # is freed by the cycle collector only, whenever that next runs. Inside a capture that destroys GPU objects
        # on the capturing thread, which the runtime answers with an abort: collect such garbage now, and keep the
        # collector out of the capture (torch.cuda.graph no longer collects on entry).
        gc.collect()
        collecting = gc.isenabled()
        gc.disable()
        try:
            pool = torch.cuda.graph_pool_handle()
            g1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1, pool=pool, capture_error_mode="thread_local"):
                self.draw()
                self.compute()
                captured = exchange_captured()
                one_graph = captured or not vqa_dp.active(self.process_group)
                if captured:
                    self.exchange()
                if one_graph:
                    self.update()
            g2 = None
            if not one_graph:
                g2 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g2, pool=pool, capture_error_mode="thread_local"):
                    self.update()
        finally:
            if collecting:
                gc.enable()
        self.graphs = (g1, g2)
        torch.cuda.synchronize(self.device)

    def draws_from(self, feed) -> bool:
        """Is `feed` the very feed this step was captured with, at the seed the graph's gather launch holds? Any
        other feed, or this one after a change of seed, has to be drawn by the caller and run eagerly."""
        return feed is self.feed and feed.seed == self.feed_seed

    def replay(self):
        g1, g2 = self.graphs
        g1.replay()
        if g2 is not None:
            self.exchange()  # the whole bucket, eagerly, between the split graphs
            g2.replay()


@contextmanager
def averaged_weights(model, store):
    """The body runs on the optimizer's moving average of `store`'s weights: the contents of the two buffers change
    places on entry and change back on exit (Adam.swap_weights, exact), also when the body raises. No pointer moves,
    so captured graphs and per-call weight images see the averaged weights inside and the trained ones after."""
    opt = model.optimizer
    if opt is None or not opt.averaging:
        raise ValueError("averaged_weights: the model's optimizer keeps no average (compile with "
                         "vqa_optim.Adam(average_decay=...))")
    if model._in_average:
        raise RuntimeError("averaged_weights: already inside the context")
    opt.swap_weights(store)
    model._in_average = True
    try:
        yield model
    finally:
        opt.swap_weights(store)
        model._in_average = False


def refuse_averaged(model, what):
    """Training and saving act on the trained weights: refused, before any launch, while they hold the average."""
    if model._in_average:
        raise RuntimeError(f"{what}: not inside averaged_weights() (the weights hold their moving average)")


def check_skip_limit(optimizer, max_consecutive_skips):
    """fit's max_consecutive_skips, checked before anything is launched: None, or an integer >= 1 with an optimizer
    that skips non-finite steps (vqa_optim.Adam(skip_nonfinite=True))."""
    if max_consecutive_skips is None:
        return
    if (isinstance(max_consecutive_skips, bool) or not isinstance(max_consecutive_skips, int)
            or max_consecutive_skips < 1):
        raise ValueError(f"max_consecutive_skips: an integer >= 1 or None (got {max_consecutive_skips!r})")
    if optimizer is None or not optimizer.skip_nonfinite:
        raise ValueError("max_consecutive_skips needs an optimizer that skips non-finite steps "
                         "(compile with vqa_optim.Adam(skip_nonfinite=True))")


def raise_on_skips(optimizer, max_consecutive_skips, epoch):
    """The epoch-end check of fit(max_consecutive_skips=...): the one read of the guard's counters."""
    if max_consecutive_skips is None:
        return
    total, row = (int(c) for c in optimizer.skipped.tolist())
    if row >= max_consecutive_skips:
        raise FloatingPointError(f"epoch {epoch + 1}: the last {row} train steps in a row were skipped for a "
                                 f"non-finite gradient (max_consecutive_skips={max_consecutive_skips}); "
                                 f"{total} steps skipped in all")


def adam_state(optimizer) -> dict:
    """The optimizer's entries of a checkpoint: both moments (host copies), the step count, when it keeps one the
    weights' moving average, and with skip_nonfinite the guard's two counters (adam_skipped: skipped in all, in a
    row)."""
    sd = {"adam_m": optimizer.m.detach().cpu().clone(), "adam_v": optimizer.v.detach().cpu().clone(),
          "iterations": int(optimizer.iterations.item())}
    if optimizer.average is not None:
        sd["adam_ema"] = optimizer.average.detach().cpu().clone()
    if optimizer.skipped is not None:
        sd["adam_skipped"] = [int(c) for c in optimizer.skipped.tolist()]
    return sd


def adam_from_checkpoint(ck, store, layout, path) -> dict:
    """Those entries of the checkpoint dict `ck`, the moments (and the average) brought into `store`'s layout."""
    sd = {"adam_m": store.from_layout(ck["adam_m"], layout, f"{path} (adam_m)"),
          "adam_v": store.from_layout(ck["adam_v"], layout, f"{path} (adam_v)"), "iterations": ck["iterations"]}
    if "adam_ema" in ck:
        sd["adam_ema"] = store.from_layout(ck["adam_ema"], layout, f"{path} (adam_ema)")
    if "adam_skipped" in ck:
        sd["adam_skipped"] = ck["adam_skipped"]
    return sd


def set_adam_state(optimizer, sd, device, store=None):
    """`store` holds the weights already loaded: an averaging optimizer given a state without an average (a file
    written without averaging) starts its average from them. An average given to an optimizer that keeps none is
    ignored. The skip counters (adam_skipped) load into a guarded optimizer, as zeros when the state has none (the
    guard's flag starts as 1); an optimizer without the guard ignores them."""
    optimizer.m.copy_(sd["adam_m"].to(device))
    optimizer.v.copy_(sd["adam_v"].to(device))
    optimizer.iterations.fill_(int(sd["iterations"]))
    if optimizer.average is not None:
        if "adam_ema" in sd:
            optimizer.average.copy_(sd["adam_ema"].to(device))
        elif store is not None:
            optimizer.average.copy_(store.flat)
    if optimizer.skipped is not None:
        total, row = (int(c) for c in sd.get("adam_skipped", (0, 0)))
        optimizer.skipped.copy_(torch.tensor([total, row], dtype=torch.int64))
        optimizer.step_ok.fill_(0 if row else 1)
