"""hipGraph instance pool: the replay policy that EAST.detect_start and TRBA.recognize_start_graph share.

Per key (whatever makes a captured sequence reusable: shapes, addresses, launch stream) a bucket holds a warm-up flag and the
instances captured so far.  The first call of a key declines (lazy one-time kernel attributes must not fall into a capture).  Later
calls take an idle instance, or capture through the owner's callable: two instances the first time (consecutive batches overlap —
submit i+1 before collect i — so both are needed), one after, none beyond MAX_INSTANCES.  The owner keeps its static buffers in
`Instance.state` and decides what is captured; nothing here launches anything but the event of a lease."""
import torch

MAX_INSTANCES = 4  # per key; a caller that holds more handles than this in flight gets eager launches for the rest


class Instance:
    __slots__ = ("graph", "state", "busy")

    def __init__(self, graph, state):
        self.graph, self.state, self.busy = graph, state, False


class Bucket:
    __slots__ = ("warm", "inst")

    def __init__(self):
        self.warm, self.inst = False, []


class Lease:
    """Holds one instance for a handle, from right behind its replay; released by the owner's finish call (also when that raises)
    or when the handle is dropped without ever being finished.  An event recorded right behind the replay says when the instance's
    static buffers may be rewritten: a dropped handle waits for THAT event only — never a device-wide synchronize from a finalizer
    (the garbage collector may run it while another stream capture is in progress, and a synchronize would invalidate that capture)."""

    def __init__(self, inst):
        self.inst = inst
        self.done = torch.cuda.Event()
        self.done.record()  # on the replay's stream, behind the replay

    def release(self):
        if self.inst is not None:
            self.inst.busy = False
            self.inst = None

    def __del__(self):
        if self.inst is None:
            return
        try:
            if torch.cuda.is_current_stream_capturing():
                return  # leave the instance marked busy: it is simply never reused (a new one is captured on demand)
            if not self.done.query():
                self.done.synchronize()
        except Exception:
            return  # the wait failed: do not hand the instance out again
        self.release()


class GraphPool:
    def __init__(self):
        self.buckets = {}  # key -> Bucket, least recently used first

    def warm(self, key, max_buckets=None):
        """Touch `key`'s bucket; False on the first call of a key, which the caller runs eagerly.  max_buckets bounds the cache for
        owners whose keys move (a key that holds a tensor's address): least recently used buckets with no instance in use go."""
        bucket = self.buckets.pop(key, None) or Bucket()
        self.buckets[key] = bucket
        while max_buckets is not None and len(self.buckets) > max_buckets:
            victim = next((k for k, b in self.buckets.items() if k != key and not any(i.busy for i in b.inst)), None)
            if victim is None:
                break
            del self.buckets[victim]
        was, bucket.warm = bucket.warm, True
        return was

    def acquire(self, key, capture):
        """An instance of a warm key, marked busy, for the caller to fill, replay and wrap in a Lease: an idle one, else a new one
        from `capture() -> (graph, state)`.  None once MAX_INSTANCES are all in use: the caller launches eagerly."""
        bucket = self.buckets[key]
        inst = next((i for i in bucket.inst if not i.busy), None)
        if inst is None:
            if len(bucket.inst) >= MAX_INSTANCES:
                return None
            for _ in range(2 if not bucket.inst else 1):
                bucket.inst.append(Instance(*capture()))
            inst = bucket.inst[-1]
        inst.busy = True
        return inst
