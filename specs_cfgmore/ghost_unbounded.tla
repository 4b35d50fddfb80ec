------------------------------ MODULE ghost_unbounded ------------------------------
(* ghost_history with an UNBOUNDED write counter: the state space is infinite without the view and finite with it.
   Small == n <= K bounds the unviewed comparison run (K = 16 in the cfg: the depth of the quotient graph). *)
EXTENDS Naturals, Sequences, TLC
CONSTANT K
(* --algorithm ghost_unbounded
variables x = 0, last = 0, n = 0;

process W \in 1..2
variable t = 0;
begin
  rd: t := x;
  wr: x := (t + 1) % 3;
      last := self;
      n := n + 1;
  ck: if x # 0 then
        goto rd;
      end if;
end process

end algorithm *)

View == <<x, pc, t>>
Small == n <= K
=============================================================================
