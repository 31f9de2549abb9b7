// Compression against preset dictionaries through the JavaScript host path
// (streams-api.mjs -> zsnapi.node -> zs_pool_deflate_batch_dict): compressBatch*(inputs,
// format, {dictionary}) with one view shared by all inputs or one per input (null = none);
// the outputs come back through decompressBatch(..., {dictionary}) and node's own zlib.
//   node deflate-dict.test.mjs cpu   -- the argument checks only (no GPU needed)
import zlib from "zlib";

import * as corpus from "../../../tests/golden/corpus.mjs";
import * as api from "../streams-api.mjs";

let checks = 0;
const expect = (c, m) => { if (!c) throw new Error("FAIL " + m); checks++; };
const same = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) === 0;

async function rejects(p, pred, what) {
  let e = null;
  try { await p; } catch (x) { e = x; }
  expect(e !== null && pred(e), what + (e ? ": " + e.message : ": no error"));
}

async function argumentChecks() {
  const one = [new Uint8Array([1, 2, 3])];
  for (const bad of ["abc", 5, {}, new ArrayBuffer(4)])
    await rejects(api.compressBatch(one, "deflate-raw", { dictionary: bad }), (e) => e instanceof TypeError,
                  "a non-view dictionary is a TypeError (" + typeof bad + ")");
  await rejects(api.compressBatch(one, "deflate-raw", { dictionary: ["abc"] }), (e) => e instanceof TypeError,
                "a non-view entry of a per-input dictionary array is a TypeError");
  await rejects(api.compressBatchSettled(one, "deflate-raw", { dictionary: [null, null] }), (e) => e instanceof TypeError,
                "a per-input dictionary array of the wrong length is a TypeError");
  await rejects(api.compressBatchDetailed(one, "deflate", { dictionary: "abc" }), (e) => e instanceof TypeError,
                "the detailed entry checks it too");
}

function adler32(b) {
  let a = 1, s = 0;
  for (let i = 0; i < b.length; i++) {
    a = (a + b[i]) % 65521;
    s = (s + a) % 65521;
  }
  return ((s << 16) | a) >>> 0;
}

async function main() {
  await argumentChecks();
  if (process.argv[2] === "cpu") {
    console.log("ok " + checks);
    return;
  }
  const dictA = corpus.text(corpus.streamSeed(900), 32768);
  const dictB = corpus.text(corpus.streamSeed(901), 257);
  const recs = [];
  for (let i = 0; i < 48; i++) recs.push(corpus.text(corpus.streamSeed(1000 + i), 100 + 61 * i));
  recs.push(new Uint8Array(0));
  const per = recs.map((r, i) => [dictA, dictB, null][i % 3]);
  for (const [format, inflate] of [["deflate", zlib.inflateSync], ["deflate-raw", zlib.inflateRawSync]]) {
    for (const level of [1, 6]) {
      // one dictionary shared by all inputs (a Uint8Array, a DataView)
      for (const d of [dictA, new DataView(dictA.buffer, dictA.byteOffset, dictA.byteLength)]) {
        const outs = await api.compressBatch(recs, format, { level, dictionary: d });
        const back = await api.decompressBatch(outs, format, { dictionary: dictA });
        back.forEach((o, i) => expect(same(o, recs[i]), `${format} L${level} shared dictionary, record ${i}`));
        outs.forEach((o, i) => expect(same(new Uint8Array(inflate(o, { dictionary: dictA })), recs[i]),
                                      `${format} L${level} shared dictionary, node's zlib, record ${i}`));
        if (format === "deflate") outs.forEach((o, i) => expect((o[1] & 0x20) !== 0, `FDICT, record ${i}`));
      }
      // one per input: A, B or none
      const outs2 = await api.compressBatch(recs, format, { level, dictionary: per });
      const back2 = await api.decompressBatch(outs2, format, { dictionary: per });
      back2.forEach((o, i) => expect(same(o, recs[i]), `${format} L${level} per-input dictionaries, record ${i}`));
      const plain = await api.compressBatch(recs, format, { level });
      outs2.forEach((o, i) => expect(per[i] !== null || same(o, plain[i]), `no dictionary: the plain bytes, record ${i}`));
      const det = await api.compressBatchDetailed(recs, format, { level, dictionary: per });
      det.outputs.forEach((o, i) => expect(det.status[i] === 1 && same(o, outs2[i]) &&
                                           det.check[i] === (format === "deflate" ? adler32(recs[i]) : 1),
                                           `${format} L${level} detailed, record ${i}`));
      const settled = await api.compressBatchSettled(recs, format, { level, dictionary: per });
      settled.forEach((s, i) => expect(s.status === "fulfilled" && same(s.value, outs2[i]), `settled ${i}`));
    }
  }
  // gzip, and level 0, with a dictionary: the stream layer's init error
  await rejects(api.compressBatch(recs, "gzip", { dictionary: dictA }), (e) => e.message === "init failed: -2",
                "gzip takes no dictionary");
  await rejects(api.compressBatch(recs, "deflate", { level: 0, dictionary: dictA }), (e) => e.message === "init failed: -2",
                "level 0 with a dictionary is not built");
  await rejects(api.compressBatchDetailed(recs, "gzip", { dictionary: dictA }), (e) => e.code === "-2", "detailed: code -2");
  const g = await api.compressBatch(recs, "gzip", { dictionary: recs.map(() => null) });
  expect(g.every((o, i) => same(new Uint8Array(zlib.gunzipSync(o)), recs[i])), "gzip with no dictionary set is the plain call");
  console.log("ok " + checks);
}

main().catch((e) => { console.error(e); process.exit(1); });
