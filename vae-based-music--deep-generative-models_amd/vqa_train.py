"""What the VQ-VAE and prior trainers share: the train step as a replayable hipGraph, and the optimizer's half of a
checkpoint. What differs between the models stays with them: their inputs and checks, and what surrounds a replay."""
from __future__ import annotations

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


def adam_state(optimizer) -> dict:
    """The optimizer's entries of a checkpoint: both moments (host copies) and the step count."""
    return {"adam_m": optimizer.m.detach().cpu().clone(), "adam_v": optimizer.v.detach().cpu().clone(),
            "iterations": int(optimizer.iterations.item())}


def adam_from_checkpoint(ck, store, layout, path) -> dict:
    """Those entries of the checkpoint dict `ck`, the moments brought into `store`'s layout."""
    return {"adam_m": store.from_layout(ck["adam_m"], layout, f"{path} (adam_m)"),
            "adam_v": store.from_layout(ck["adam_v"], layout, f"{path} (adam_v)"), "iterations": ck["iterations"]}


def set_adam_state(optimizer, sd, device):
    optimizer.m.copy_(sd["adam_m"].to(device))
    optimizer.v.copy_(sd["adam_v"].to(device))
    optimizer.iterations.fill_(int(sd["iterations"]))
