"""Point-to-point transports for the halo exchange.

The reference's ``HaloUpdater`` needs exactly ``Isend`` / ``Irecv`` of contiguous 1-D buffers plus
``Get_rank`` / ``Get_size`` (util/pace/util/comm.py:14-73, halo_updater.py:241-267).  Two transports provide that
over device tensors:

* ``TorchDistComm``  -- one process per GPU, ``torch.distributed`` (backend "nccl" is RCCL over xGMI; "gloo" is used by
  the CPU tests).  ``exchange`` posts all sends and receives of one halo update as ONE ``batch_isend_irecv`` group,
  so RCCL sees a single grouped launch per update and the transfers run on RCCL's stream while the compute stream
  keeps launching kernels until ``wait``.
* ``ThreadComm``     -- several tiles inside one process (one Python thread per tile, e.g. all six tiles of a small
  cubed sphere on a single 288 GB device).  A send enqueues a device-side copy; a receive copies it out.
* ``DeviceCubeComm`` -- ``ThreadComm`` for the whole cubed sphere on one device (``run_cube``): the six ranks of a halo update
  meet in a rendezvous, and the last one to arrive launches ONE kernel that reads every neighbour's field and writes every
  halo (``pace_halo_cube``, pace_amd/util/halo.py).  No message, no buffer.

``ThreadComm.rendezvous`` is the collective behind gather and scatter (pace_amd/util/gather.py): every rank posts, the last one
to arrive acts for all of them -- under ``DeviceCubeComm`` with ONE ``pace_cube_gather`` / ``pace_cube_scatter`` launch.
"""
import threading
from collections import defaultdict, deque

import torch


class Request:
    def __init__(self, fn=None):
        self._fn = fn

    def wait(self):
        if self._fn is not None:
            self._fn()
            self._fn = None


class TorchDistComm:
    def __init__(self, group=None):
        import torch.distributed as dist

        if not dist.is_initialized():
            raise RuntimeError("torch.distributed is not initialised (launch with torch.distributed.run)")
        self._dist = dist
        self._group = group

    def Get_rank(self):
        return self._dist.get_rank(self._group)

    def Get_size(self):
        return self._dist.get_world_size(self._group)

    def barrier(self):
        self._dist.barrier(self._group)

    def exchange(self, sends, recvs, tag=0):
        """sends / recvs: lists of (1-D tensor, peer rank).  Returns a Request."""
        dist = self._dist
        ops = [dist.P2POp(dist.irecv, buf, peer, self._group, tag) for buf, peer in recvs]
        ops += [dist.P2POp(dist.isend, buf, peer, self._group, tag) for buf, peer in sends]
        works = dist.batch_isend_irecv(ops)

        def fin():
            for w in works:
                w.wait()

        return Request(fin)

    def allreduce_min(self, value: float) -> float:
        t = torch.tensor([value], dtype=torch.float64, device="cuda" if self._dist.get_backend(self._group) == "nccl" else "cpu")
        self._dist.all_reduce(t, op=self._dist.ReduceOp.MIN, group=self._group)
        return float(t.item())

    def allreduce_sum_u64(self, values):
        """The wrapping (mod 2^64) sum over the ranks of each of `values`: an int64 SUM, which wraps the same way."""
        import numpy as np

        a = np.ascontiguousarray(values, dtype=np.uint64)
        t = torch.from_numpy(a.view(np.int64).copy())
        if self._dist.get_backend(self._group) == "nccl":
            t = t.cuda()
        self._dist.all_reduce(t, op=self._dist.ReduceOp.SUM, group=self._group)
        return t.cpu().numpy().view(np.uint64)

    def allreduce_fixed_point(self, words, finalize, stream=None):
        """The energy fixer's global sum (pace_amd/fv3core/stencils/energy_fixer.py): `words`, this rank's int64 tensor of
        fixed-point words, becomes the sum over the ranks by ONE int64 all_reduce(SUM) in place -- on the device under "nccl", no
        copy to the host -- and ``finalize([words])`` makes this rank's finalising launch.  -> what finalize returned."""
        self._dist.all_reduce(words, op=self._dist.ReduceOp.SUM, group=self._group)
        return finalize([words])

    def allreduce_level_max(self, cmax, finalize, stream=None):
        """The tracer advection's Courant numbers per level (pace_amd/fv3core/stencils/tracer_2d_1l.py): `cmax`, this rank's
        float64 tensor of one maximum per level, becomes the maximum over the ranks by ONE all_reduce(MAX) in place -- on the
        device under "nccl" -- and ``finalize([cmax])`` makes this rank's pace_tracer_subcycles launch and its one transfer.
        The reduction runs on the bit patterns (the same memory viewed as int64): every value is >= 0, so the patterns order
        like the values, and a NaN, which a floating-point MAX may drop, is the largest of them.  -> what finalize returned."""
        self._dist.all_reduce(cmax.view(torch.int64), op=self._dist.ReduceOp.MAX, group=self._group)
        return finalize([cmax])


class NullComm:
    """util/pace/util/null_comm.py:15-80: the rank of a communicator that has no peers -- what it "receives" is a fill value
    (zero as in the reference's Irecv; halo updates therefore zero the halos).  Lets one tile's operators run alone, as the
    reference's own drop-in test does (tests/main/fv3core/test_dycore_call.py)."""

    def __init__(self, rank, total_ranks, fill_value=0.0):
        self.rank, self.total_ranks, self._fill_value = rank, total_ranks, fill_value

    def __repr__(self):
        return f"NullComm(rank={self.rank}, total_ranks={self.total_ranks})"

    def Get_rank(self):
        return self.rank

    def Get_size(self):
        return self.total_ranks

    def barrier(self):
        return

    def exchange(self, sends, recvs, tag=0):
        def fin():
            for buf, _peer in recvs:
                buf[:] = 0.0  # NullAsyncResult.wait (null_comm.py:11-13)

        return Request(fin)

    def allreduce_min(self, value: float) -> float:
        return value

    def allreduce_sum_u64(self, values):
        """None: a rank alone cannot know the sum over the globe."""
        return None

    def allreduce_fixed_point(self, words, finalize, stream=None):
        """The rank's own tile only: a rank alone cannot know the sum over the globe, so the "global" sum of the energy fixer
        is this tile's.  It is what lets one tile's LagrangianToEulerian run alone with consv_te > 0."""
        return finalize([words])

    def allreduce_level_max(self, cmax, finalize, stream=None):
        """The rank's own tile only, as allreduce_fixed_point: one tile's TracerAdvection sub-cycles by its own Courant numbers."""
        return finalize([cmax])


class LoopbackComm(NullComm):
    """NOT a reference communicator: a lone rank that receives from each peer what it sent to that peer (the cube's messages
    are symmetric in size).  The halos then hold values of the right magnitude -- not the neighbour's, and not in the
    neighbour's orientation -- so that one tile's step can be TIMED alone without the zeros of NullComm turning the state
    into NaNs (tools/dycore_bench.py --single).  Never used for results."""

    def exchange(self, sends, recvs, tag=0):
        sent = {peer: buf for buf, peer in sends}

        def fin():
            for buf, peer in recvs:
                src = sent.get(peer)
                if src is None or src.numel() != buf.numel():
                    buf[:] = 0.0
                else:
                    buf.copy_(src)

        return Request(fin)


class _World:
    """Shared state of the tile threads.  The condition's lock doubles as a run token: a tile thread holds it whenever it
    executes and gives it up only while it waits for a message (``Condition.wait_for`` releases and re-acquires it), so the
    tiles run as coroutines -- one at a time, in message-driven order -- and nothing below (PyTorch, the HIP runtime, the
    library) is ever entered from two threads at once."""

    def __init__(self, n):
        self.n = n
        self.cond = threading.Condition()  # RLock inside: re-entrant
        self.mail = defaultdict(deque)
        self.arrived = 0
        self.generation = 0
        self.failed = False
        self.reduce_arrived = 0
        self.reduce_generation = 0
        self.reduce_sum = None
        self.reduce_result = None
        # DeviceCubeComm's rendezvous of the halo updates: (tag, generation) -> {rank: what it posted}, and -> number of ranks
        # that have still to wait() for a launch that has been issued
        self.halo_posts = {}
        self.halo_issued = {}
        # ThreadComm.rendezvous: (tag, generation) -> {rank: payload}, and -> [result, ranks that have still to take it]
        self.meet_posts = {}
        self.meet_results = {}


class ThreadComm:
    def __init__(self, world: _World, rank: int):
        self._world = world
        self._rank = rank
        self._meet_generation = defaultdict(int)  # tag -> rendezvous this rank has joined under it

    def Get_rank(self):
        return self._rank

    def Get_size(self):
        return self._world.n

    def _wait(self, predicate, what):
        w = self._world
        if not w.cond.wait_for(lambda: predicate() or w.failed, timeout=600):
            raise TimeoutError(f"tile {self._rank} waiting for {what}")
        if w.failed and not predicate():
            raise RuntimeError(f"tile {self._rank}: another tile failed while this one waited for {what}")

    def barrier(self):
        w = self._world
        with w.cond:
            gen = w.generation
            w.arrived += 1
            if w.arrived == w.n:
                w.arrived = 0
                w.generation += 1
                w.cond.notify_all()
            else:
                self._wait(lambda: w.generation != gen, "barrier")

    def allreduce_sum_u64(self, values):
        """The wrapping (mod 2^64) sum over the tiles of each of `values`, through the world object."""
        import numpy as np

        a = np.array(values, dtype=np.uint64)
        w = self._world
        with w.cond:
            gen = w.reduce_generation
            w.reduce_sum = a if w.reduce_arrived == 0 else w.reduce_sum + a  # (unsigned array addition wraps)
            w.reduce_arrived += 1
            if w.reduce_arrived == w.n:
                # (the next reduction cannot complete, and replace the result, before every tile has left this one)
                w.reduce_result, w.reduce_arrived = w.reduce_sum, 0
                w.reduce_generation += 1
                w.cond.notify_all()
            else:
                self._wait(lambda: w.reduce_generation != gen, "allreduce_sum_u64")
            return w.reduce_result.copy()

    def allreduce_fixed_point(self, words, finalize, stream=None):
        """The energy fixer's global sum through the host, as allreduce_sum_u64: the words of every tile are summed there (the
        wrapping unsigned sum is the signed sum), written back into `words`, and every rank makes its own finalising launch."""
        import numpy as np

        total = self.allreduce_sum_u64(words.cpu().numpy().view(np.uint64))
        words.copy_(torch.from_numpy(total.view(np.int64).copy()))
        return finalize([words])

    def allreduce_level_max(self, cmax, finalize, stream=None):
        """The Courant numbers per level through the host, as allreduce_sum_u64: the maximum over the tiles of the bit patterns
        (values >= 0 order like their patterns; a NaN is the largest) is written back into `cmax`, and every rank makes its own
        pace_tracer_subcycles launch and transfer."""
        import numpy as np

        def last(posts):
            return np.maximum.reduce([posts[r] for r in sorted(posts)])

        total = self.rendezvous("allreduce_level_max", cmax.cpu().numpy().view(np.uint64).copy(), last)
        cmax.copy_(torch.from_numpy(total.view(np.float64).copy()))
        return finalize([cmax])

    def rendezvous(self, tag, payload, last):
        """The collective of gather and scatter (pace_amd/util/gather.py): every rank posts `payload` under `tag`; the last one
        to arrive runs ``last({rank: payload})`` -- for DeviceCubeComm that is the one launch for the whole cube -- and every
        rank returns what it returned.  The n-th call under a tag on one rank meets the n-th on the others."""
        w = self._world
        with w.cond:
            gen = self._meet_generation[tag]
            self._meet_generation[tag] += 1
            ticket = (tag, gen)
            posts = w.meet_posts.setdefault(ticket, {})
            posts[self._rank] = payload
            if len(posts) == w.n:
                del w.meet_posts[ticket]
                w.meet_results[ticket] = [last(posts), w.n]
                w.cond.notify_all()
            else:
                self._wait(lambda: ticket in w.meet_results, f"rendezvous {ticket}")
            entry = w.meet_results[ticket]
            entry[1] -= 1
            if entry[1] == 0:
                del w.meet_results[ticket]
            return entry[0]

    def exchange(self, sends, recvs, tag=0):
        w = self._world
        with w.cond:
            for buf, peer in sends:
                w.mail[(self._rank, peer, tag)].append(buf.clone())
            w.cond.notify_all()

        def fin():
            for buf, peer in recvs:
                key = (peer, self._rank, tag)
                with w.cond:
                    self._wait(lambda: len(w.mail[key]) > 0, f"message {key}")
                    data = w.mail[key].popleft()
                buf.copy_(data)

        return Request(fin)


class DeviceCubeComm(ThreadComm):
    """A rank of the whole cubed sphere on one device.  Everything of ThreadComm is inherited; on top of it the ranks of one
    halo update (same tag, same generation: the n-th update of that tag on every rank) meet here.  ``snapshot``: the ranks
    behave exactly as ThreadComm's (pack at start(), buffers, unpack at wait()), which keeps the reference's contract that a
    field may be rewritten after start()."""

    def __init__(self, world: _World, rank: int, snapshot: bool = False):
        super().__init__(world, rank)
        self.snapshot = bool(snapshot)
        self._halo_generation = defaultdict(int)  # tag -> updates this rank has started under it

    def allreduce_fixed_point(self, words, finalize, stream=None):
        """The energy fixer's global sum with no copy at all: a rendezvous, and the last rank to arrive makes the ONE finalising
        launch over the six tiles' word buffers in tile order.  Every rank returns what that launch's finalize returned (the one
        buffer of results, which every rank's next kernel reads).  The tiles' launches that filled the words and the finalising
        launch must be ordered by one stream, as a fused halo update's."""
        def last(posts):
            order = sorted(posts)
            streams = [posts[r][1] for r in order]
            if len(set(streams)) != 1:
                raise RuntimeError(f"the tiles of a fused global sum launched on different streams ({streams}): the one "
                                   "finalising launch is ordered behind one stream only")
            return finalize([posts[r][0] for r in order])

        return self.rendezvous("allreduce_fixed_point", (words, getattr(stream, "value", stream)), last)

    def allreduce_level_max(self, cmax, finalize, stream=None):
        """The Courant numbers per level with ONE launch and ONE transfer for the cube: a rendezvous, and the last rank to
        arrive makes the pace_tracer_subcycles launch over the six tiles' buffers in tile order and the transfer of its nk + 2
        integers.  Every rank returns the same host array.  One stream must order the tiles' launches, as for the fixed-point
        sum."""
        def last(posts):
            order = sorted(posts)
            streams = [posts[r][1] for r in order]
            if len(set(streams)) != 1:
                raise RuntimeError(f"the tiles of a fused level maximum launched on different streams ({streams}): the one "
                                   "finalising launch is ordered behind one stream only")
            return finalize([posts[r][0] for r in order])

        return self.rendezvous("allreduce_level_max", (cmax, getattr(stream, "value", stream)), last)

    def halo_post(self, tag, payload):
        """Post this rank's part of the next update under `tag`.  Returns (ticket, posts): posts is None unless this rank is
        the last of the world to post -- then it is {rank: payload} of all of them, and the caller launches the update and
        reports it with halo_issue(ticket)."""
        w = self._world
        with w.cond:
            ticket = (tag, self._halo_generation[tag])
            self._halo_generation[tag] += 1
            posts = w.halo_posts.setdefault(ticket, {})
            posts[self._rank] = payload
            if len(posts) < w.n:
                return ticket, None
            del w.halo_posts[ticket]
            return ticket, posts

    def halo_issue(self, ticket):
        w = self._world
        with w.cond:
            w.halo_issued[ticket] = w.n
            w.cond.notify_all()

    def halo_wait(self, ticket):
        """Block (yielding the run token, as ThreadComm._wait does) until the launch of `ticket` has been issued."""
        w = self._world
        with w.cond:
            self._wait(lambda: ticket in w.halo_issued, f"halo update {ticket}")
            w.halo_issued[ticket] -= 1
            if w.halo_issued[ticket] == 0:
                del w.halo_issued[ticket]


def run_tiles(n, fn):
    """Run ``fn(comm)`` for n tiles on n threads of this process; returns their results in tile order."""
    return _run_world(n, fn, ThreadComm)


def run_cube(fn, snapshot=False):
    """Run ``fn(comm)`` for the six tiles of the cubed sphere on six threads of this process, all on the current device, with
    DeviceCubeComm ranks: a halo update is one kernel launch for the whole cube.  Between start() and wait() of an update a rank
    must not write the fields it handed over, nor rely on their halos (the data moves when the LAST tile has started); a caller
    that cannot keep that passes snapshot=True.  Returns the results in tile order."""
    return _run_world(6, fn, lambda world, r: DeviceCubeComm(world, r, snapshot=snapshot))


def _run_world(n, fn, make_comm):
    world = _World(n)
    results, errors = [None] * n, []
    # the current device is a per-thread setting: hand the caller's on to the tile threads (a rank of a multi-GPU run owns
    # device LOCAL_RANK, and a new thread would start on device 0).  Nothing here initialises the GPU.
    device = None
    try:
        import torch

        if torch.cuda.is_initialized():
            device = torch.cuda.current_device()
    except Exception:  # noqa: BLE001
        device = None

    def target(r):
        if device is not None:
            import torch

            torch.cuda.set_device(device)
        with world.cond:  # the run token (see _World)
            try:
                results[r] = fn(make_comm(world, r))
            except BaseException as e:  # noqa: BLE001
                import traceback

                errors.append((r, e, traceback.format_exc()))
                world.failed = True
                world.cond.notify_all()

    threads = [threading.Thread(target=target, args=(r,), daemon=True, name=f"tile{r}") for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        r, e, tb = errors[0]
        raise RuntimeError(f"tile {r} failed: {e!r}\n{tb}") from e
    return results
