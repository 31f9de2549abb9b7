// BGZF files through the JavaScript host path (streams-api.mjs -> zsnapi.node -> zs_pool_inflate_batch_bgzf):
// decompressBatch*(inputs, "gzip", {members: "bgzf"}) on blocks built here around node's own raw deflate, with and
// without outCapacity, a block whose ISIZE lies beside a good file, and the rejection rules.
//   node inflate-bgzf.test.mjs cpu   -- the argument checks and bgzfOutLength only (no GPU needed)
import zlib from "zlib";

import * as corpus from "../../../tests/golden/corpus.mjs";
import * as api from "../streams-api.mjs";

let checks = 0;
const expect = (c, m) => { if (!c) throw new Error("FAIL " + m); checks++; };
const same = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) === 0;
const EOF = new Uint8Array(Buffer.from("1f8b08040000000000ff0600424302001b0003000000000000000000", "hex"));
const cat = (parts) => new Uint8Array(Buffer.concat(parts.map((p) => Buffer.from(p.buffer, p.byteOffset, p.length))));

// node has no crc32 before 20.15 / 22.2: the trailer's value from a gzip member of the same data
function block(data, isize = data.length) {
  const buf = Buffer.from(data.buffer, data.byteOffset, data.length);
  const raw = zlib.deflateRawSync(buf, { level: 6 });
  const gz = zlib.gzipSync(buf);
  const b = Buffer.alloc(18 + raw.length + 8);
  Buffer.from("1f8b08040000000000ff0600424302000000", "hex").copy(b, 0);
  b.writeUInt16LE(b.length - 1, 16);
  raw.copy(b, 18);
  gz.copy(b, 18 + raw.length, gz.length - 8, gz.length - 4);
  b.writeUInt32LE(isize, b.length - 4);
  return new Uint8Array(b);
}
const bgzf = (x, size) => {
  const parts = [];
  for (let a = 0; a < x.length; a += size) parts.push(block(x.subarray(a, Math.min(a + size, x.length))));
  return cat([...parts, EOF]);
};

async function rejects(p, pred, what) {
  let e = null;
  try { await p; } catch (x) { e = x; }
  expect(e !== null && pred(e), what + (e ? ": " + e.message : ": no error"));
}

async function argumentChecks() {
  const x = corpus.text(corpus.streamSeed(5), 1000);
  const file = bgzf(x, 300);
  const one = [file];
  const type = (e) => e instanceof TypeError;
  const ok = { outCapacity: 1000, members: "bgzf" };
  for (const format of ["deflate", "deflate-raw", "deflate64-raw"])
    await rejects(api.decompressBatch(one, format, ok), type, format + ": a TypeError");
  await rejects(api.decompressBatch(one, "gzip", { members: "BGZF" }), type, "another word: a TypeError");
  await rejects(api.decompressBatchSettled(one, "gzip", { ...ok, dictionary: new Uint8Array(4) }), type, "with a dictionary: a TypeError");
  await rejects(api.decompressBatchDetailed(one, "gzip", { ...ok, restartPoints: "scan" }), type, "with restartPoints: a TypeError");
  // the sizing: host arithmetic over the headers
  expect(api.bgzfOutLength(file) === 1000 && api.bgzfOutLength(EOF) === 0, "bgzfOutLength of truthful files");
  const plain = new Uint8Array(zlib.gzipSync(Buffer.from("abc")));
  expect(api.bgzfOutLength(plain) === null && api.bgzfOutLength(cat([block(x.subarray(0, 10)), plain])) === null &&
         api.bgzfOutLength(file.subarray(0, file.length - 40)) === null && api.bgzfOutLength(new Uint8Array(0)) === null,
         "bgzfOutLength of a plain member, a mixed chain, a truncated block, nothing");
  await rejects(api.decompressBatch([file, cat([block(x.subarray(0, 10)), plain])], "gzip", { members: "bgzf" }),
                (e) => type(e) && /input 1 is not BGZF throughout: give outCapacity/.test(e.message), "without outCapacity, not BGZF: a TypeError");
}

async function main() {
  await argumentChecks();
  if (process.argv[2] === "cpu") {
    console.log("ok " + checks);
    return;
  }
  const x = corpus.text(corpus.streamSeed(79), 150000);
  const a = bgzf(x, 65280);
  const b = cat([block(x.subarray(0, 100)), block(x.subarray(100, 101)), EOF, new Uint8Array(13)]);  // then padding
  const mixed = cat([block(x.subarray(0, 100)), new Uint8Array(zlib.gzipSync(Buffer.from(x.buffer, x.byteOffset + 100, 50))), EOF]);
  // sized from the headers
  const outs = await api.decompressBatch([a, b], "gzip", { members: "bgzf" });
  expect(same(outs[0], x) && same(outs[1], x.subarray(0, 101)), "two files, no outCapacity");
  // with capacities: field for field what members: true gives
  const options = { outCapacity: [150000, 104, 152] };
  const d = await api.decompressBatchDetailed([a, b, mixed], "gzip", { ...options, members: "bgzf" });
  const m = await api.decompressBatchDetailed([a, b, mixed], "gzip", { ...options, members: true });
  expect(d.status.every((s) => s === 1) && d.consumed[0] === a.length && d.consumed[1] === b.length - 13, "consumed: behind the last trailer");
  for (const k of ["status", "phase", "consumed", "check"]) expect(String(Array.from(d[k])) === String(Array.from(m[k])), k + " as members: true");
  expect(d.outputs.every((o, i) => same(o, m.outputs[i])) && same(d.outputs[2], x.subarray(0, 150)), "outputs as members: true");
  // an ISIZE one too small in the second block fails that input alone: "incorrect length check"
  const lie = cat([block(x.subarray(0, 100)), block(x.subarray(100, 300), 199), block(x.subarray(300, 400)), EOF]);
  const s = await api.decompressBatchSettled([lie, b], "gzip", { outCapacity: [400, 104], members: "bgzf" });
  expect(s[0].status === "rejected" && s[0].reason.message === "process error: -3" && s[0].reason.zmsg === "incorrect length check",
         "the lying block's error");
  expect(s[1].status === "fulfilled" && same(s[1].value, x.subarray(0, 101)), "the neighbour of a lying file");
  // a total that does not fit is the caller's capacity
  const t = await api.decompressBatchSettled([a], "gzip", { outCapacity: 149999, members: "bgzf" });
  expect(t[0].status === "rejected" && t[0].reason.zmsg === "output capacity exceeded", "the capacity outcome");
  console.log("ok " + checks);
}

main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
