"""The component arrangements the general encoder tests share (test_encoder_model_cpu.py, test_encoder_components_gpu.py): each as
an encoder_model.Arrangement, and its translation into the library's jpgpu_encode_description."""
import numpy as np

import encoder_model as em

LUM75, CHR75 = em.scale_by_quality(em.STD_LUMINANCE, 75), em.scale_by_quality(em.STD_CHROMINANCE, 75)
LUM40, CHR90 = em.scale_by_quality(em.STD_LUMINANCE, 40), em.scale_by_quality(em.STD_CHROMINANCE, 90)

# name -> sampling factors (h, v) in AddComponent order
SAMPLING = {
    "A": [(1, 1)] * 4,
    "B": [(2, 2), (1, 1), (1, 1)],
    "C": [(2, 2), (2, 1), (1, 2)],
    "D": [(4, 2), (2, 1), (1, 1)],
    "E": [(1, 1), (2, 2), (2, 2)],
    "F": [(2, 1), (1, 2)],
    "J": [(4, 4)] * 4,
}
SIZES = {"A": [(37, 29), (264, 136)], "B": [(90, 41)], "C": [(90, 41), (33, 17)], "D": [(100, 50), (8, 8)],
         "E": [(264, 136), (24, 24), (8, 8)], "F": [(40, 24)], "J": [(70, 40), (32, 32)]}


def arrangement(name, built=False, restart_interval=0, most_optimal=False):
    """The first component on quantisation table 0 and Huffman tables 0, the others on tables 1 (A: the fourth back on 0) -- for
    B that is the EncodeAction arrangement itself."""
    std = [None] * 4 if built else em.standard_tables()
    comps = []
    for k, (h, v) in enumerate(SAMPLING[name]):
        t = 0 if k in (0, 3) else 1
        comps.append(em.Component(k + 1, t, t, t, h, v, LUM75 if t == 0 else CHR75))
    return em.Arrangement(comps, [(0, LUM75), (1, CHR75)], [(0, 0, std[0]), (1, 0, std[1]), (0, 1, std[2]), (1, 1, std[3])], restart_interval,
                          most_optimal)


def identifiers(name, built=False):
    """H: componentIndex 7, 9, 200; quantisation identifiers 2 and 3 plus a third table nobody uses; Huffman identifiers 3 and 1, AC set
    before DC; quantisation table 2 replaced after AddComponent captured it (the DQT carries the new one)."""
    std = [None] * 4 if built else em.standard_tables()
    comps = []
    for k, (h, v) in enumerate(SAMPLING[name]):
        t = 0 if k == 0 else 1
        comps.append(em.Component((7, 9, 200, 201)[k], (2, 3)[t], (3, 1)[t], (3, 1)[t], h, v, LUM75 if t == 0 else CHR75))
    return em.Arrangement(comps, [(2, LUM40), (3, CHR75), (0, CHR90)], [(1, 3, std[1]), (0, 3, std[0]), (1, 1, std[3]), (0, 1, std[2])])


def shared_tables(name):
    """G: every component on Huffman tables 0, both to be built: the counts add up."""
    a = arrangement(name, built=True)
    for c in a.components:
        c.dc_id = c.ac_id = 0
    a.huffman_tables = [(0, 0, None), (1, 0, None)]
    return a


def dc_given_ac_built(name):
    std = em.standard_tables()
    a = arrangement(name)
    a.huffman_tables = [(0, 0, std[0]), (1, 0, None), (0, 1, std[2]), (1, 1, None)]
    return a


def unused_builder(name):
    a = arrangement(name)
    a.huffman_tables = a.huffman_tables + [(1, 2, None)]
    return a


def pixels(width, height, samples, seed):
    return np.random.default_rng(seed).integers(0, 256, (height, width, samples)).astype(np.uint8)


def to_description(arr, width, height, in_components=None, input_rgb=0):
    from jpeglibrary_amd import encoder

    return encoder.describe(width, height, [(c.component_index, c.h, c.v, c.quant_id, c.dc_id, c.ac_id, c.quant) for c in arr.components],
                            arr.quant_tables, arr.huffman_tables, in_components=in_components, input_rgb=input_rgb,
                            restart_interval=arr.restart_interval, most_optimal_coding=arr.most_optimal)
