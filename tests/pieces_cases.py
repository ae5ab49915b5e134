"""Cut lists for the tests of zjni_compress_pieces_batch_device (tests/test_emu_pieces.py on the CPU, tests/test_gpu_pieces.py on the GPU): the rules of
include/zjni_amd.h restated in plain Python, one list of every illegal kind, and the layout of d_cut / d_cut_off for a call."""


def bound(s):
    """ZSTD_COMPRESSBOUND"""
    return s + (s >> 8) + (((128 << 10) - s) >> 11 if s < (128 << 10) else 0)


def legal(size, cuts, chunk, off_ascends=True):
    if not off_ascends:
        return False
    if not all(0 < c < size for c in cuts):
        return False
    if any(b <= a for a, b in zip(cuts[:-1], cuts[1:])):
        return False
    edges = [0] + list(cuts) + [size]
    return all(b - a <= chunk for a, b in zip(edges[:-1], edges[1:]))


def illegal(chunk):
    """name -> (buffer size, cuts, d_cut_off ascends at the buffer): one buffer of every illegal kind, sizes up to 3 * chunk"""
    return {
        "not_ascending": (900, [300, 200, 600], True),
        "equal_neighbour": (900, [300, 300, 600], True),
        "equal_neighbour_far_lane": (900, list(range(1, 70)) + [69] + list(range(70, 100)), True),      # one lane of the wave's second round sees it, no other
        "cut_of_zero": (900, [0, 400], True),
        "cut_equal_to_size": (900, [400, 900], True),
        "cut_beyond_size": (900, [400, 901], True),
        "piece_above_chunk_first": (chunk + 500, [chunk + 1], True),
        "piece_above_chunk_middle": (3 * chunk, [500, 500 + chunk + 1, 2 * chunk + 600], True),
        "piece_above_chunk_last": (2 * chunk + 1, [chunk], True),
        "no_cut_above_chunk": (chunk + 1, [], True),
        "cut_off_descends": (900, [300, 600], False),
        "empty_with_a_cut": (0, [0], True),
        "empty_with_cuts": (0, [1, 2], True),
    }


def lay_out(lists):
    """lists: (cuts, d_cut_off ascends) per buffer -> (d_cut, d_cut_off[n + 1]) as Python lists.  A buffer's list begins where its predecessor's ends, so after a
    buffer at which d_cut_off descends the lists go on at a lower address: the runs of lists between two descents are laid out from the top of the array
    downwards, one free word between them."""
    runs = [[]]
    for cuts, asc in lists:
        runs[-1].append((cuts, asc))
        if not asc:
            runs.append([])
    lens = [sum(len(cuts) for cuts, asc in run if asc) for run in runs]
    top = sum(lens) + len(runs) + 3
    flat, cut_off = [77] * top, []
    for run, total in zip(runs, lens):
        pos = top = top - total - 1
        cut_off.append(pos)                                   # buffer 0's beginning, or the end of the buffer that closed the run before: lower than its beginning
        for cuts, asc in run:
            if asc:
                flat[pos:pos + len(cuts)] = [int(c) for c in cuts]
                pos += len(cuts)
                cut_off.append(pos)
    assert len(cut_off) == len(lists) + 1
    return flat, cut_off
