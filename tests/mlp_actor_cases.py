"""The shapes tests/test_gpu_mlp_actor.py runs mdr_mlp_actor_sample on, and the inputs it builds for them - on the CPU, so that
tests/test_mlp_actor.py can judge those inputs without a kernel."""
from tests import actor_ref as ar

# (F, (H1, H2)): one per shape edge of csrc/mdr_mlp_actor.hip
SHAPES = [
    (51, (256, 256)),       # the reference's net
    (121, (256, 256)),      # the widest observation of the reference
    (128, (256, 256)),      # the widest input the kernel takes
    (65, (256, 256)),       # the first F past the 64-feature form
    (64, (255, 241)),       # partial last blocks in both layers
    (51, (129, 130)),       # just past FusedActor
    (7, (16, 256)),         # waves that own no unit of layer 1
    (1, (1, 1)),
]
BATCHES = (1, 17, 1029)     # each ends in a partial tile of 32
NET_SEED, NET_SCALE, NET_KEEP = 3, 2.0, 8      # scale 2: p0 spans about 0.003 .. 0.997 (at 1 only 0.39 .. 0.67 - a weak check)
ROWS_SEED = 5


def shape_id(shape):
    return "%d-%dx%d" % (shape[0], shape[1][0], shape[1][1])


def make_actor(shape):
    """The ActorMLP of a shape, on the CPU."""
    return ar.make_actor(shape[0], shape[1], seed=NET_SEED, scale=NET_SCALE, keep=NET_KEEP)


def rows(shape, A):
    """float32 [A, F] rows on the CPU."""
    return ar.rows_inputs(shape[0], A, seed=ROWS_SEED)
