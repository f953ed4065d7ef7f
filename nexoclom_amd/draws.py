"""How the packets of a run are drawn, stated once per sampler kind.  WHICH Outputs and chunks
exist is distributed.pass_plan's and chunk_plan's business; when they are launched, the callers'."""
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from itertools import islice

import numpy as np

from .Output import Output, fresh_key
from .source_distribution import WindowGenerator


class Draws:
    """sampler='numpy' (``on_host``: threads can draw ahead of the device): Output k is drawn from
    default_rng(seed + k), from fresh entropy without a seed.  'device' with 'philox' (``one_key``):
    one key for the run, counter-based on the global packet index; an unseeded run gets a fresh
    key (recorded; not key 0 every run).  'device' with 'pcg64': the device follows the host's
    streams.  Ranks that share a run (``cp``) need one seed even for the host: rank 0's."""

    def __init__(self, sampler, generator, seed, cp=None):
        self.on_host, self.generator = sampler != 'device', generator
        self.one_key = not self.on_host and generator != 'pcg64'
        shared = cp is not None and cp.world > 1
        if seed is None and (shared or not self.on_host):
            seed = int.from_bytes(os.urandom(4), 'little') if self.on_host else fresh_key()
            if shared:
                seed = int.from_bytes(cp.bcast_bytes(seed.to_bytes(8, 'little'), 8), 'little')
        self.seed, self.lead = seed, None

    def seed_of(self, k):
        return self.seed if self.one_key or self.seed is None else self.seed + k

    def output_keywords(self, entry, presampled):
        """For a distributed.PlannedOutput; ``presampled``: its launch group draws for it."""
        device = {} if self.on_host else dict(
            sampler='device', generator=self.generator, first_index=entry.first_index,
            presampled=presampled, materialize_x0=not presampled)
        return dict(seed=self.seed_of(entry.call_number), **device)

    def fill_group(self, context, outs):
        """Make the packets of ``outs`` the resident set.  (The host's: integrate_batch uploads.)"""
        lead, size = outs[0], outs[0].npackets
        if self.one_key:        # consecutive slices of one counter space: one call draws them all
            soa = context.sample_packets(size*len(outs), self.seed, lead._first_index,
                                         download=True, **lead.source_desc())
            for g, out in enumerate(outs):
                out._adopt_x0(soa[:, g*size:(g + 1)*size])
        elif not self.on_host:  # each follows its own seeded stream: a piece of the set each
            src = lead.source_desc()
            for g, out in enumerate(outs):
                out._adopt_x0(context.sample_packets(
                    size, out.device_key, lead._first_index, download=True, pcg64=(size, 0),
                    piece=(g*size, size*len(outs)), **src))

    def chunk_output(self, inputs, ctx, piece):
        """The Output of a ``piece`` of chunk_plan.  The host draws only the rows [a, b) a rank owns
        (PCG64.advance: bit-identical to slicing the whole draw) or, where that cannot be, the whole
        chunk.  The device draws the rows in place; its first Output stands for the later chunks."""
        k, c0, clen, a, b = piece
        window = None if self.one_key else (clen, a - c0, b - c0)     # (one counter space)
        if self.on_host:
            cut = self.seed is not None and window != (clen, 0, clen) \
                and WindowGenerator.windowable(inputs)
            return Output(inputs, clen, seed=self.seed_of(k), window=window if cut else None,
                          integrate=False, save=False, context=ctx)
        if self.lead is None:
            self.lead = Output(inputs, clen if window else b - a, seed=self.seed_of(k),
                               integrate=False, save=False, context=ctx, sampler='device',
                               generator=self.generator, window=window, first_index=a,
                               materialize_x0=False)
            self.src = self.lead.source_desc()
        else:                   # same inputs: no need to rebuild the tables
            ctx.sample_packets(b - a, self.seed_of(k), a, **self.src,
                               **self.lead.stream_window(self.seed_of(k), window))
        return self.lead

    def upload_chunk(self, ctx, out, piece):
        """Rows [a, b) of a host-drawn chunk's Output to the device."""
        if self.on_host:
            soa, (_, c0, _, a, b) = out.x0_soa(), piece
            ctx.upload_soa(soa if soa.shape[1] == b - a
                           else np.ascontiguousarray(soa[:, a - c0:b - c0]))


class DrawAhead(deque):
    """``job(item)`` for every item on a thread pool, submitted in order and only as far ahead as
the caller says (``fill``); the deque holds the jobs on their way, in that order."""

    def __init__(self, job, items, threads):
        super().__init__()
        self.pool = ThreadPoolExecutor(max_workers=threads)
        self._jobs = (self.pool.submit(job, item) for item in items)

    def fill(self, window):
        self.extend(islice(self._jobs, max(0, window - len(self))))
